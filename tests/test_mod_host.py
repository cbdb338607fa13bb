"""The burst modulator (sfe_dsp_mod_*) without a GPU: the C ABI's declarations and exports, the host plan -- the reference
of the device's bits -- against an independent numpy restatement of the law (synth.mod_symbols, synth.mod_reference: the
symbols in float32 exactly as the law forms them, the sum in float64), bit for bit on dyadic inputs and within the
direct-sum bound on general ones, the coded bits against the encoder, the shapes, the placement, the transmit wire format,
every refusal of plan, the loopback through the receive blocks' references, and the build lists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mod_checks as mc
from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
MOD_FUNCS = ("sfe_dsp_mod_footprint", "sfe_dsp_mod_plan", "sfe_dsp_mod_create", "sfe_dsp_mod_process_stream", "sfe_dsp_mod_destroy")
F32 = np.float32
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


def coded_bits(api, K, gen, keep, terminated, data, n_info):
    """The burst's coded bits by the encoder the library already has (uncoded: the payload bits)."""
    bits = mc.payload_bits(data, n_info)
    return bits if gen is None else api.vit_encode(K, gen, bits, keep, terminated)


def restated_stream(api, data, n_info, taps, sps, K=7, gen=None, keep=None, terminated=True, order=2, preamble=None, amp=1.0, n_out=0,
                    start_base=0, start_step=0, absolute=False):
    """The stream by the restatement, complex128: every frame summed in float64 and laid at its place, zeros elsewhere."""
    y = np.zeros(n_out, np.complex128)
    for b, row in enumerate(np.atleast_2d(data)):
        s = synth.mod_symbols(coded_bits(api, K, gen, keep, terminated, row, n_info), order, amp, preamble)
        f = synth.mod_reference(s, taps, sps, absolute=absolute)
        y[start_base + b * start_step:][:f.size] = f
    return y


def words(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_header_declares_mod_abi_and_library_exports_it(L):
    declared = set(re.findall(r"\b(sfe_dsp_mod_[a-z0-9_]+)\s*\(", open(HDR).read()))
    assert declared == set(MOD_FUNCS)
    for name in MOD_FUNCS:
        assert hasattr(L.load(), name), name
        assert name in L.SIGNATURES, name


def test_build_lists_name_the_mod_files():
    from simplefe_amd import build
    assert "api_mod.hip" in build.HOST_SOURCES and "mod.hip" in build.EXACT_SOURCES and build.SCRATCH_FREE["mod.hip"]
    assert build.KERNEL_FILES["mod"][:2] == ("mod.hip", "mod.h")
    assert "mod.hip" in open(os.path.join(ROOT, "CMakeLists.txt")).read()


def test_footprint(api):
    tile, lds = api.mod_footprint()
    assert tile >= 256 and tile % 2 == 0 and 0 < lds <= 65536


# ---- the coded bits: a one-tap pulse of 1 at sps 1 with amp 1 hands the symbols through
@pytest.mark.parametrize("code", mc.CODES + [(7, None)], ids=mc.CODE_IDS + ["uncoded"])
@pytest.mark.parametrize("terminated", [True, False], ids=["terminated", "truncated"])
def test_coded_bits_equal_the_encoder(api, code, terminated):
    K, gen = code
    a4 = F32(np.float64(1.0) / np.sqrt(np.float64(2.0)))
    for n_info in (1, 5, 64, 200):
        data = mc.payload_bytes(n_info, 1, 7 * n_info + K)[0]
        for keep in (None, mc.PUNCT[len(gen)]) if gen else (None,):
            want = coded_bits(api, K, gen, keep, terminated, data, n_info)
            for order in (2, 4):
                N, F, n_soft = api.mod_plan(K, gen, n_info, [1.0], 1, keep, terminated, order)
                assert n_soft == want.size and N == (want.size if order == 2 else (want.size + 1) // 2) and F == N
                y = api.mod_plan(K, gen, n_info, [1.0], 1, keep, terminated, order, data=data, n_out=F)
                if order == 2:
                    assert np.array_equal(words(y.real), words(np.where(want == 1, F32(-1), F32(1)))) and not words(y.imag).any()
                else:
                    padded = np.concatenate([want, np.zeros(want.size & 1, np.uint8)])
                    assert np.array_equal(words(y.real), words(np.where(padded[0::2] == 1, -a4, a4)))
                    assert np.array_equal(words(y.imag), words(np.where(padded[1::2] == 1, -a4, a4)))


def test_an_odd_n_soft_takes_the_pad(api):
    """K = 3 truncated at n_info 5, punctured to 7 kept positions: the fourth QPSK symbol's imaginary part is the 0 bit's."""
    N, F, n_soft = api.mod_plan(3, (7, 5), 5, [1.0], 1, mc.PUNCT[2], False, 4)
    assert (n_soft, N) == (7, 4)
    y = api.mod_plan(3, (7, 5), 5, [1.0], 1, mc.PUNCT[2], False, 4, data=[0xF8], n_out=4)
    assert y.imag[3] > 0


# ---- dyadic inputs: every partial sum is exact, so the plan equals the float64 restatement bit for bit
SHAPES = [(1, 1, 0), (2, 3, 1), (10, 3, 32), (4, 7, 1), (10, 161, 32), (64, 3, 0), (1, 64, 1), (2, 128, 32), (64, 4096, 1)]


def dyadic_taps(n, seed):
    return (np.random.default_rng(seed).integers(-1024, 1025, size=n) / 1024.0).astype(F32)


def dyadic_preamble(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.integers(-64, 65, size=n) + 1j * rng.integers(-64, 65, size=n)) / 64.0).astype(np.complex64)


@pytest.mark.parametrize("shape", SHAPES, ids=["sps%d-taps%d-pre%d" % s for s in SHAPES])
def test_dyadic_inputs_equal_the_restatement_bit_for_bit(api, shape):
    """BPSK at amp 0.5: symbols are multiples of 2^-7 below 1, taps multiples of 2^-10, at most 64 terms: every partial sum
    is a multiple of 2^-17 of at most 2^5 -- 22 bits -- so float32 holds it exactly.  This pins arm, halo, puncture numbering."""
    sps, n_taps, Lp = shape
    K, gen, n_info, keep = 7, (0o171, 0o133), 45, mc.PUNCT[2]
    taps, pre = dyadic_taps(n_taps, 11 + n_taps), dyadic_preamble(Lp, 5 + Lp)
    data = mc.payload_bytes(n_info, 3, 17 + sps)
    N, F, n_soft = api.mod_plan(K, gen, n_info, taps, sps, keep, preamble=pre, amp=0.5)
    Q = -(-n_taps // sps)
    assert N == Lp + n_soft and F == (N + Q - 1) * sps
    kw = dict(K=K, gen=gen, keep=keep, preamble=pre, amp=0.5, n_out=3 * (F + 3) + 9, start_base=5, start_step=F + 3)
    got = api.mod_plan(n_info=n_info, taps=taps, sps=sps, data=data, **kw)
    want = restated_stream(api, data, n_info, taps, sps, **kw).astype(np.complex64)
    assert np.array_equal(words(got), words(want))
    assert not words(got[:5]).any() and not words(got[5 + 2 * (F + 3) + F:]).any()      # +0, not -0, where no frame lies


# ---- general inputs: the direct-sum bound
@pytest.mark.parametrize("order", [2, 4], ids=["bpsk", "qpsk"])
@pytest.mark.parametrize("pulse", ["raised-cosine", "random"])
def test_general_inputs_stay_inside_the_direct_sum_bound(api, order, pulse):
    """|plan - float64| <= (Q + 1) 2^-24 A per component, A the same sum on |h| and |s|: a chain of Q fused multiply-adds
    rounds Q times, each by at most 2^-24 of a partial sum that A bounds (tests/stream_checks.py: direct_bound)."""
    sps, K, gen, n_info = 10, 7, (0o171, 0o133), 106
    taps = mc.rc_taps(sps, 8) if pulse == "raised-cosine" else np.random.default_rng(3).standard_normal(157).astype(F32)
    pre = synth.psk_symbols(32, 4, seed=8).astype(np.complex64)
    data = mc.payload_bytes(n_info, 2, 23)
    N, F, _ = api.mod_plan(K, gen, n_info, taps, sps, order=order, preamble=pre, amp=0.7)
    Q = -(-taps.size // sps)
    kw = dict(K=K, gen=gen, order=order, preamble=pre, amp=0.7, n_out=2 * F + 11, start_base=4, start_step=F)
    got = api.mod_plan(n_info=n_info, taps=taps, sps=sps, data=data, **kw).astype(np.complex128)
    ref = restated_stream(api, data, n_info, taps, sps, **kw)
    A = restated_stream(api, data, n_info, taps, sps, absolute=True, **kw)
    for g, r, a in ((got.real, ref.real, A.real), (got.imag, ref.imag, A.imag)):
        err, bound = np.abs(g - r), (Q + 1) * U24 * a
        print(pulse, order, "worst error / bound", float(np.max(err / np.maximum(bound, 1e-300))))
        assert (err <= bound).all()


# ---- placement
def test_placement(api):
    """start_step = F exactly and F + 3, an odd start_base, a tail behind the last frame, and no bursts at all."""
    sps, taps, n_info = 4, dyadic_taps(7, 2), 20
    data = mc.payload_bytes(n_info, 3, 31)
    N, F, _ = api.mod_plan(7, None, n_info, taps, sps, amp=0.5)
    one = [api.mod_plan(7, None, n_info, taps, sps, amp=0.5, data=data[b], n_out=F) for b in range(3)]
    for step, base, tail in ((F, 0, 0), (F, 7, 0), (F + 3, 13, 21)):
        n_out = base + 2 * step + F + tail
        y = api.mod_plan(7, None, n_info, taps, sps, amp=0.5, data=data, n_out=n_out, start_base=base, start_step=step)
        covered = np.zeros(n_out, bool)
        for b in range(3):
            assert np.array_equal(words(y[base + b * step:][:F]), words(one[b]))
            covered[base + b * step:][:F] = True
        assert not words(y[~covered]).any()
    assert not words(api.mod_plan(7, None, n_info, taps, sps, amp=0.5, data=np.zeros((0, 3), np.uint8), n_out=37)).any()


def test_a_symmetric_pulse_puts_symbol_k_at_k_sps_plus_half_its_length(api):
    taps = mc.rc_taps(10, 8)
    y = api.mod_plan(7, None, 8, taps, 10, data=[0b10110010], n_out=(8 + 16) * 10)
    assert np.array_equal(y.real[80::10][:8], np.where(mc.payload_bits([0b10110010], 8) == 1, F32(-1), F32(1)))


# ---- the transmit wire format
@pytest.mark.parametrize("base", [0, 7], ids=["even-offset", "odd-offset"])
def test_tx10_bytes_are_the_converters_of_the_f32_output(api, L, base):
    """|y| < 1; with an odd o_b a frame starts in the middle of a 5-byte group."""
    c = mc.CHAIN
    taps, pre, data, _ = mc.chain_parts()
    kw = dict(preamble=pre, data=data[:2], n_out=2 * c["F"] + 30 + 2 * base, start_base=base, start_step=c["F"] + 9, **mc.chain_plan_kwargs())
    y = api.mod_plan(taps=taps, **kw)
    assert np.abs(y.view(F32)).max() < 1.0
    tx = api.mod_plan(taps=taps, out_fmt=L.FMT_TX10, **kw)
    assert tx.size == kw["n_out"] // 2 * 5 and np.array_equal(tx, synth.tx10_pack(y))


# ---- refusals
def plan_rc(L, **over):
    a = dict(K=7, n_gen=2, gen=(0o171, 0o133), keep=None, P=1, terminated=1, n_info=64, order=2, pre=[1, 0, 0, 1], n_pre=2, sps=4,
             taps=[0.5, 1, 0.5], n_taps=3, amp=1.0, fmt=0, data=bytes(16), in_stride=8, n_bursts=0, base=0, step=0, n_out=0, out=None)
    a.update(over)
    gen = None if a["gen"] is None else (C.c_uint32 * len(a["gen"]))(*a["gen"])
    keep = None if a["keep"] is None else (C.c_uint8 * len(a["keep"]))(*a["keep"])
    pre = None if a["pre"] is None else (C.c_float * len(a["pre"]))(*a["pre"])
    taps = None if a["taps"] is None else (C.c_float * len(a["taps"]))(*a["taps"])
    data = None if a["data"] is None else (C.c_uint8 * len(a["data"])).from_buffer_copy(a["data"])
    N, F, ns = C.c_int(-1), C.c_int(-1), C.c_size_t(99)
    rc = L.load().sfe_dsp_mod_plan(a["K"], a["n_gen"], gen, keep, a["P"], a["terminated"], a["n_info"], a["order"], pre, a["n_pre"], a["sps"], taps,
                                   a["n_taps"], a["amp"], a["fmt"], data, a["in_stride"], a["n_bursts"], a["base"], a["step"], a["n_out"], a["out"],
                                   C.byref(N), C.byref(F), C.byref(ns))
    return rc, N.value, F.value, ns.value


def test_every_refusal_of_plan(L):
    lib = L.load()
    assert plan_rc(L) == (L.SFE_OK, 2 + 140, (142 + 1 - 1) * 4, 140)
    nan, inf = float("nan"), float("inf")
    shapes = [dict(K=2), dict(K=10), dict(n_gen=1), dict(n_gen=5, gen=(1, 1, 1, 1, 1)), dict(gen=None), dict(gen=(0, 1)), dict(gen=(128, 1)),
              dict(terminated=2), dict(n_info=0), dict(n_info=8193), dict(n_info=-1), dict(keep=(1, 1), P=0), dict(keep=(1,) * 66, P=33),
              dict(keep=(0, 0), P=1), dict(keep=(2, 1), P=1), dict(n_gen=0, n_info=0), dict(n_gen=0, n_info=8193),
              dict(order=1), dict(order=3), dict(order=8), dict(amp=0.0), dict(amp=-1.0), dict(amp=nan), dict(amp=inf),
              dict(n_pre=-1), dict(n_pre=4097), dict(pre=None), dict(pre=[1, nan, 0, 1]), dict(pre=[1, 0, inf, 1]),
              dict(sps=0), dict(sps=65), dict(n_taps=0), dict(n_taps=65, sps=1, taps=[1.0] * 65),
              dict(taps=None), dict(taps=[0.5, nan, 0.5]), dict(taps=[0.5, 1, -inf]), dict(fmt=1), dict(fmt=3)]
    for over in shapes:
        rc, N, F, ns = plan_rc(L, **over)
        assert (rc, N, F, ns) == (L.SFE_EINVAL, 0, 0, 0), over
        assert lib.sfe_dsp_last_error().startswith(b"mod: "), (over, lib.sfe_dsp_last_error())
    F = 568
    places = [dict(n_bursts=1, base=-1, n_out=2 * F), dict(n_bursts=2, base=0, step=F - 1, n_out=4 * F), dict(n_bursts=2, base=1, step=F, n_out=2 * F),
              dict(n_bursts=1, base=0, n_out=F - 1), dict(n_bursts=0, n_out=1 << 31), dict(n_bursts=1 << 31, n_out=8), dict(fmt=2, n_bursts=0, n_out=7),
              dict(n_bursts=2, base=0, step=1 << 62, n_out=4 * F), dict(n_bursts=1, base=0, n_out=F, data=None)]
    for over in places:
        rc, N, Fr, ns = plan_rc(L, **over)
        assert (rc, N, Fr, ns) == (L.SFE_EINVAL, 142, F, 140), over
        assert lib.sfe_dsp_last_error().startswith(b"mod: "), over
    assert plan_rc(L, n_bursts=2, base=0, step=F, n_out=2 * F, in_stride=7)[0] == L.SFE_ERANGE
    # what is allowed: one burst whatever start_step says, frames that touch, an uncoded shape with the code's arguments unset
    assert plan_rc(L, n_bursts=1, base=3, step=-5, n_out=F + 3)[0] == L.SFE_OK
    assert plan_rc(L, n_bursts=2, base=0, step=F, n_out=2 * F)[0] == L.SFE_OK
    assert plan_rc(L, n_gen=0, gen=None, K=0, terminated=7, P=0, n_pre=0, pre=None) == (L.SFE_OK, 64, 64 * 4, 64)
    assert plan_rc(L, n_taps=64, sps=1, taps=[1.0] * 64, n_pre=0, pre=None) == (L.SFE_OK, 140, 140 + 63, 140)


def test_create_refuses_bad_shapes_on_any_machine(api, L):
    with pytest.raises(api.SfeError) as e:
        api.Mod(7, (0o171, 0o133), 64, [1.0], 0)
    assert e.value.code == L.SFE_EINVAL and "mod: " in str(e.value)
    with pytest.raises(api.SfeError) as e:
        api.Mod(7, (0o171, 0o133), 64, [1.0], 1, order=3)
    assert e.value.code == L.SFE_EINVAL


# ---- the loopback's inputs are decodable by the references alone
@pytest.mark.parametrize("fmt", ["f32", "tx10-as-u8"])
def test_cpu_loopback(api, L, fmt):
    """The plan's waveform for the chain shape through synth.corr_reference, api.burst_plan and api.vit_plan: the
    transmitted bytes, count 0, statuses 0 -- and the correlator's peaks where the law puts symbol 0."""
    c = mc.CHAIN
    taps, pre, data, tpl = mc.chain_parts()
    n_out = c["n_bursts"] * c["step"]
    kw = dict(preamble=pre, data=data, n_out=n_out, start_base=c["base"], start_step=c["step"], **mc.chain_plan_kwargs())
    N, F, n_soft = api.mod_plan(c["K"], c["gen"], c["n_info"], taps, c["sps"], preamble=pre, amp=c["amp"])
    assert (N, F, n_soft) == (c["N"], c["F"], 224)
    if fmt == "f32":
        x = api.mod_plan(taps=taps, **kw)
    else:
        x = synth.u8_to_cf32(mc.tx10_as_u8_samples(api.mod_plan(taps=taps, out_fmt=L.FMT_TX10, **kw)))
    _, val, idx = synth.corr_reference(x, tpl, c["step"], c["min_energy"])
    assert idx[0].tolist() == [c["base"] + c["tpl_at"] + c["tpl_len"] - 1] * c["n_bursts"]
    sym, rec, st = api.burst_plan(pre, c["sps"], c["N"], c["lag"], x=x, idx=idx[0], gate=val[0], start_base=-(c["tpl_len"] - 1), start_step=c["step"])
    by, vrec, vst = api.vit_plan(c["K"], c["gen"], c["n_info"], in_mode=L.VIT_IN_BPSK, skip=c["Lp"], x=sym, status_in=st)
    print(fmt, "burst statuses", st, "vit statuses", vst, "counts", vrec[:, 1])
    assert not st.any() and not vst.any() and not vrec[:, 1].any()
    assert np.array_equal(by, data)
