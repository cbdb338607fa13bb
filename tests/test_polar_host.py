"""The FM, phase and envelope detector (sfe_dsp_polar_*) without a GPU: the C ABI's declarations and exports, the build
lists, the refusals of the plan and of create, the host plan against an exact restatement of the law (rational arithmetic,
one rounding per operation) and against the float64 reference synth.polar_reference, the exact values, a tone, cuts and
the carried sample, and the kernels' resources.

The bars (include/sfe_dsp.h), with gain = 1 (a gain that is no power of two adds one rounding of y):
    PM  |y - atan2| <= 2 ulp(pi) = 4.77e-7 rad        at scales 1, 1e-20 and 1e20, on the unit-circle grid and on noise
    FM  |y - angle of the exact product| <= 3 ulp(pi) = 7.15e-7 rad
    AM  |y - |x|| <= 1.3e-7 |x|
FM and AM square the samples in float32, so their law holds where a square is a normal float32: their three scales are 1,
1e-9 and 1e9 (squares at 1e-18 and 1e18); at 1e20 a square overflows and at 1e-20 it is a denormal with a few bits, which
is the law's range and not its error.  Every measured worst error is printed beside its bar."""
import ctypes as C
import json
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
POLAR_FUNCS = ("sfe_dsp_polar_plan", "sfe_dsp_polar_create", "sfe_dsp_polar_set_input_format", "sfe_dsp_polar_process_stream",
               "sfe_dsp_polar_reset", "sfe_dsp_polar_destroy")
FM, PM, AM = synth.POLAR_FM, synth.POLAR_PM, synth.POLAR_AM
ULP_PI = 2.0 ** -22
BAR = {PM: 2 * ULP_PI, FM: 3 * ULP_PI, AM: 1.3e-7}
PI_2, PI = np.float32(float.fromhex("0x1.921fb6p+0")), np.float32(float.fromhex("0x1.921fb6p+1"))
COEF = [float.fromhex(h) for h in ("0x1.fffffcp-1", "-0x1.555390p-2", "0x1.995304p-3", "-0x1.2215e6p-3", "0x1.ae613cp-4",
                                   "-0x1.28e046p-4", "0x1.46db72p-5", "-0x1.d9c858p-7", "0x1.43849ep-9")]


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ ABI and build lists
def test_header_declares_polar_abi_and_library_exports_it(L):
    from simplefe_amd import lib
    hdr = open(HDR).read()
    assert set(re.findall(r"\b(sfe_dsp_polar_[a-z0-9_]+)\s*\(", hdr)) == set(POLAR_FUNCS)
    for name in POLAR_FUNCS:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name
    for name, v in (("SFE_POLAR_FM", 0), ("SFE_POLAR_PM", 1), ("SFE_POLAR_AM", 2)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr), name
    assert (lib.POLAR_FM, lib.POLAR_PM, lib.POLAR_AM) == (0, 1, 2) == (FM, PM, AM)


def test_polar_sources_are_in_the_build_lists():
    from simplefe_amd import build
    assert "polar.hip" in build.EXACT_SOURCES and "api_polar.hip" in build.HOST_SOURCES
    assert build.KERNEL_FILES["polar"] == ("polar.hip", "polar.h", "polar_law.h", "common.h")
    assert build.SCRATCH_FREE["polar.hip"] == "detector"
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert re.search(r"set\(SFE_EXACT_SOURCES [^)]*\bpolar\.hip\b", cm)
    for f in build.KERNEL_FILES["polar"] + ("api_polar.hip",):
        assert os.path.exists(os.path.join(build.CSRC, f)), f
    # one law, compiled by both sides
    for f in ("polar.hip", "api_polar.hip"):
        assert '#include "polar_law.h"' in open(os.path.join(build.CSRC, f)).read(), f


def test_polar_kernels_use_no_scratch_and_no_lds():
    from simplefe_amd import build
    build.build_lib()
    res = json.load(open(os.path.join(build.HERE, "build", "polar.hip.resources.json")))
    inst = {tuple(a.strip() for a in re.search(r"polar_kernel<(.*?)>", k).group(1).split(",")) for k in res if "polar_kernel<" in k}
    assert inst == {(str(m), u) for m in range(3) for u in ("false", "true")}
    for k, v in res.items():
        assert v.get("ScratchSize", 1) == 0 and v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0, (k, v)
        assert v.get("LDS Size", 1) == 0, (k, v)


# ------------------------------------------------------------------------------------------------ refusals
def _plan_raw(L, mode, gain, fmt, x, n, out):
    return L.sfe_dsp_polar_plan(mode, gain, fmt, x, n, None, out)


def test_plan_refusals_carry_the_prefix(L):
    from simplefe_amd import lib
    x = np.zeros(8, np.float32)
    y = np.full(4, 7.0, np.float32)
    px, py = x.ctypes.data, y.ctypes.data_as(lib.fp)
    for why, args in (("mode 3", (3, 1.0, lib.FMT_F32, px, 4, py)), ("mode -1", (-1, 1.0, lib.FMT_F32, px, 4, py)),
                      ("the TX10 format", (FM, 1.0, lib.FMT_TX10, px, 4, py)), ("format 9", (FM, 1.0, 9, px, 4, py)),
                      ("a NaN gain", (PM, float("nan"), lib.FMT_F32, px, 4, py)), ("an infinite gain", (AM, float("inf"), lib.FMT_F32, px, 4, py)),
                      ("a null input", (FM, 1.0, lib.FMT_F32, None, 4, py)), ("a null output", (FM, 1.0, lib.FMT_F32, px, 4, None))):
        assert _plan_raw(L, *args) == lib.SFE_EINVAL, why
        assert L.sfe_dsp_last_error().startswith(b"polar: "), (why, L.sfe_dsp_last_error())
    assert np.array_equal(y, np.full(4, 7.0, np.float32))
    assert _plan_raw(L, FM, 1.0, lib.FMT_F32, None, 0, None) == lib.SFE_OK         # n_in = 0 is a no-op


@pytest.mark.parametrize("why,args", [("mode 3", (3, 1.0, 1)), ("mode -1", (-1, 1.0, 1)), ("no stream", (FM, 1.0, 0)),
                                      ("a negative count", (FM, 1.0, -2)), ("a NaN gain", (PM, float("nan"), 1)),
                                      ("an infinite gain", (AM, float("-inf"), 2))])
def test_create_refuses_before_it_looks_for_a_device(L, why, args):
    from simplefe_amd import lib
    h = C.c_void_p()
    assert L.sfe_dsp_polar_create(*args, 0, C.byref(h)) == lib.SFE_EINVAL, why
    assert L.sfe_dsp_last_error().startswith(b"polar: ") and not h.value, (why, L.sfe_dsp_last_error())


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: create succeeds there")
def test_create_without_gpu_is_enodev(L):
    from simplefe_amd import api, lib
    for mode in (FM, PM, AM):
        with pytest.raises(lib.SfeError) as e:
            api.Polar(mode, 0.5, n_streams=3)
        assert e.value.code == lib.SFE_ENODEV


def test_null_handles_are_refused(L):
    from simplefe_amd import lib
    k = C.c_size_t(5)
    assert L.sfe_dsp_polar_set_input_format(None, lib.FMT_U8) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"polar: ")
    assert L.sfe_dsp_polar_process_stream(None, None, 4, 4, None, 4, C.byref(k), None) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"polar_process_stream: ") and k.value == 0
    assert L.sfe_dsp_polar_reset(None) == lib.SFE_EINVAL and L.sfe_dsp_polar_destroy(None) == lib.SFE_OK


# ------------------------------------------------------------------------------------------------ the law, exactly
def _rn(q):
    """The float32 nearest to the rational q, ties to even, denormals included (no overflow here); as a Fraction."""
    if q == 0:
        return Fraction(0)
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    m = a / ulp
    n = m.numerator // m.denominator
    rem = m - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return (n * ulp) if q > 0 else -(n * ulp)


def _at2_exact(y, x):
    """polar_law.h's at2 in rational arithmetic with one float32 rounding per operation; float32 in, float out."""
    fy, fx = Fraction(float(y)), Fraction(float(x))
    ax, ay = abs(fx), abs(fy)
    mx, mn = max(ax, ay), min(ax, ay)
    z = Fraction(0) if mx == 0 else _rn(mn / mx)
    s = _rn(z * z)
    q = Fraction(COEF[8])
    for c in COEF[7::-1]:
        q = _rn(q * s + Fraction(c))
    r = _rn(q * z)
    if ay > ax:
        r = _rn(Fraction(float(PI_2)) - r)
    if fx < 0:
        r = _rn(Fraction(float(PI)) - r)
    if fy < 0:
        r = -r
    return float(r)


def _fm_exact(x, p):
    xr, xi, pr, pi = (Fraction(float(v)) for v in (x.real, x.imag, p.real, p.imag))
    re = _rn(xr * pr + _rn(xi * pi))
    im = _rn(xi * pr - _rn(xr * pi))
    return _at2_exact(np.float32(float(im)), np.float32(float(re)))


def _at2(api, y, x):
    """at2(y, x) through the plan: PM of x + jy, gain 1."""
    z = (np.asarray(x, np.float32) + 1j * np.asarray(y, np.float32)).astype(np.complex64)
    return api.polar_plan(z, PM, 1.0)[0]


def test_the_plan_is_the_law_operation_by_operation(api):
    rng = np.random.default_rng(synth.SEED)
    n = 1500
    z = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    z[:300] *= np.float32(1e-20)
    z[300:600] *= np.float32(1e20)
    z[600:700] = (z[600:700].real * np.float32(1e-3) + 1j * z[600:700].imag).astype(np.complex64)      # near the axes
    z[700:800] = (z[700:800].real + 1j * z[700:800].imag * np.float32(1e-4)).astype(np.complex64)
    z[800:900] = (z[800:900].real * (1 + 1j) * (1 + rng.integers(-2, 3, 100) * 2.0 ** -23)).astype(np.complex64)   # near the diagonals
    pm = api.polar_plan(z, PM, 1.0)[0]
    want = np.array([_at2_exact(v.imag, v.real) for v in z], np.float32)
    assert np.array_equal(_bits(pm), _bits(want))
    w = z[600:1500]
    fm = api.polar_plan(w, FM, 1.0)[0]
    want = np.array([_fm_exact(w[i], w[i - 1] if i else np.complex64(0)) for i in range(w.size)], np.float32)
    assert np.array_equal(_bits(fm), _bits(want))
    am = api.polar_plan(w, AM, 1.0)[0]
    sq = [_rn(Fraction(float(v.real)) ** 2 + _rn(Fraction(float(v.imag)) ** 2)) for v in w]
    want = np.array([np.float32(math.sqrt(float(q))) for q in sq], np.float32)      # float64's root rounds to float32's
    assert np.array_equal(_bits(am), _bits(want))
    # gain multiplies once, last
    g = np.float32(0.7)
    assert np.array_equal(_bits(api.polar_plan(w, FM, g)[0]), _bits(g * fm))
    assert np.array_equal(_bits(api.polar_plan(w, AM, g)[0]), _bits(g * am))


def test_exact_values(api):
    y = np.array([0, 0, 1, -1, 0, 1, -0.0, -0.0, 0, -1], np.float32)
    x = np.array([0, 1, 0, 0, -1, 1, -1, 1, -0.0, -1], np.float32)
    got = _at2(api, y, x)
    q = np.float32(_at2_exact(np.float32(1), np.float32(1)))
    assert abs(float(q) - math.pi / 4) <= 2.0 ** -24                              # (1, 1): the polynomial at z = 1, half an ulp from pi/4
    want = np.array([0.0, 0.0, PI_2, -PI_2, PI, q, PI, 0.0, 0.0, -(PI - q)], np.float32)     # -0 counts as not below 0
    assert np.array_equal(_bits(got), _bits(want)), (got, want)
    assert _bits(want)[0] == 0 and _bits(PI_2)[0] == 0x3FC90FDB and _bits(PI)[0] == 0x40490FDB
    # a denormal pair: the quotient is the correctly rounded 0.1 (1e-40 / 1e-39 as float32 denormals, not 0.1 itself)
    yd, xd = np.float32(1e-40), np.float32(1e-39)
    assert 0 < float(yd) < 2.0 ** -126 and 0 < float(xd) < 2.0 ** -126
    zq = np.float32(float(_rn(Fraction(float(yd)) / Fraction(float(xd)))))
    assert abs(float(zq) - 0.1) < 1e-5
    got = _at2(api, [yd], [xd])
    assert np.array_equal(_bits(got), _bits(_at2(api, [zq], [np.float32(1)])))
    assert np.array_equal(_bits(got), _bits([_at2_exact(yd, xd)])) and abs(float(got[0]) - math.atan(0.1)) < 1e-5
    # FM's first output on a fresh stream is +0 whatever the sample; AM of 3 + 4j is 5
    for v in (1 + 1j, -2 - 3j, -1 + 0j):
        assert _bits(api.polar_plan(np.array([v], np.complex64), FM, -1.5)[0])[0] in (0, 0x80000000)
    assert _bits(api.polar_plan(np.array([-2 - 3j], np.complex64), FM, 1.5)[0])[0] == 0
    assert api.polar_plan(np.array([3 + 4j], np.complex64), AM, 2.0)[0][0] == 10.0


# ------------------------------------------------------------------------------------------------ against float64
def _points():
    """name -> (complex64 points, the modes they are for)."""
    rng = np.random.default_rng(synth.SEED + 1)
    n = 1 << 20
    base = (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    k = np.arange(1 << 21)
    th = 2.0 * np.pi * k / (1 << 21)
    out = {"scale 1": (base.astype(np.complex64), (PM, FM, AM)),
           "scale 1e-20": ((base * 1e-20).astype(np.complex64), (PM,)), "scale 1e20": ((base * 1e20).astype(np.complex64), (PM,)),
           "scale 1e-9": ((base * 1e-9).astype(np.complex64), (FM, AM)), "scale 1e9": ((base * 1e9).astype(np.complex64), (FM, AM)),
           "unit circle, 2^21": ((np.cos(th) + 1j * np.sin(th)).astype(np.complex64), (PM, FM, AM)),
           "synth_cf32 noise": (synth.synth_cf32(1 << 20).view(np.complex64), (PM, FM, AM))}
    return out


@pytest.fixture(scope="module")
def points():
    return _points()


@pytest.mark.parametrize("mode", [PM, FM, AM])
def test_plan_against_the_float64_reference(api, points, mode):
    name = {PM: "PM", FM: "FM", AM: "AM"}[mode]
    worst_all = 0.0
    for tag, (z, modes) in points.items():
        if mode not in modes:
            continue
        y = api.polar_plan(z, mode, 1.0)[0].astype(np.float64)
        ref = synth.polar_reference(z, mode, 1.0)
        assert np.isfinite(y).all(), tag
        if mode == AM:
            ok = ref > 0
            err = np.abs(y[ok] - ref[ok]) / ref[ok]
            assert (y[~ok] == 0).all()
        else:
            err = np.abs(y - ref)
            err = np.minimum(err, 2 * np.pi - err)          # +pi and -pi are one angle
        worst = float(err.max())
        worst_all = max(worst_all, worst)
        print("polar %s, %s: worst error %.3e (bar %.3e, %.2f of it)" % (name, tag, worst, BAR[mode], worst / BAR[mode]))
        assert worst <= BAR[mode], (name, tag, worst, BAR[mode])
    print("polar %s: worst error over all points %.3e, bar %.3e" % (name, worst_all, BAR[mode]))


def test_reference_is_the_plain_statement():
    x = np.array([1 + 0j, 1j, -1 + 0j, -1j, 3 + 4j], np.complex64)
    assert np.allclose(synth.polar_reference(x, PM, 2.0), [0, np.pi, 2 * np.pi, -np.pi, 2 * math.atan2(4, 3)], atol=1e-15)
    assert np.allclose(synth.polar_reference(x, AM, 0.5), [0.5, 0.5, 0.5, 0.5, 2.5], atol=1e-15)
    fm = synth.polar_reference(x, FM)
    assert fm[0] == 0 and np.allclose(fm[1:4], np.pi / 2, atol=1e-15)
    assert np.allclose(synth.polar_reference(x, FM, prev=-1j)[0], np.pi / 2, atol=1e-15)
    two = synth.polar_reference(np.stack([x, x[::-1]]), FM, prev=[0, 1])
    assert two.shape == (2, 5) and np.allclose(two[0], fm, atol=1e-15) and abs(two[1, 0] - math.atan2(4, 3)) < 1e-15


@pytest.mark.parametrize("f", [0.01, 0.123456, -0.3, 0.49])
def test_a_tone_gives_its_frequency(api, f):
    n, gain = 4096, 2.0                         # a power of two: the gain rounds nothing
    x = (0.8 * np.exp(2j * np.pi * f * np.arange(n))).astype(np.complex64)
    y = api.polar_plan(x, FM, gain)[0].astype(np.float64)
    bar = gain * BAR[FM]                        # the FM bar in the output's units; the tone's own float32 rounding fits in it
    worst = np.abs(y[1:] - gain * 2 * np.pi * f).max()
    print("polar tone f = %g: worst |y - gain 2 pi f| %.3e (bar %.3e)" % (f, worst, bar))
    assert y[0] == 0 and worst <= bar, (f, worst, bar)


# ------------------------------------------------------------------------------------------------ cuts, the carried sample
@pytest.mark.parametrize("mode", [FM, PM, AM])
def test_plan_cuts_and_the_carried_sample(api, mode):
    n = 3000
    x = synth.synth_cf32(n, ch=5).view(np.complex64)
    one, last = api.polar_plan(x, mode, 0.7)
    assert last == x[-1]
    cuts, pos = [1, 3, 1020, 5, 1, 2, 4, 1023, 941], 0
    assert sum(cuts) == n
    prev, parts = None, []
    for c in cuts:
        y, prev = api.polar_plan(x[pos:pos + c], mode, 0.7, prev=prev)
        assert prev == x[pos + c - 1]
        parts.append(y)
        pos += c
    assert np.array_equal(_bits(np.concatenate(parts)), _bits(one))
    # the carried sample is what stands before the call: a stream that starts in mid-air
    y, _ = api.polar_plan(x[100:200], mode, 0.7, prev=x[99])
    assert np.array_equal(_bits(y), _bits(one[100:200]))
    if mode == FM:
        assert not np.array_equal(_bits(api.polar_plan(x[100:200], mode, 0.7)[0][:1]), _bits(one[100:101]))
    # an empty call changes nothing
    y, p = api.polar_plan(x[:0], mode, 0.7, prev=x[7])
    assert y.size == 0 and p == x[7]


@pytest.mark.parametrize("mode", [FM, PM, AM])
def test_plan_u8_equals_cf32_on_the_converted_samples(api, mode):
    n = 2049
    b = synth.offset_bytes(n, seed=11)
    b[:8] = [128, 128, 0, 255, 255, 0, 128, 127]                  # a zero sample, the corners
    want, last = api.polar_plan(synth.u8_to_cf32(b), mode, 1.3)
    got, last8 = api.polar_plan(b, mode, 1.3, in_u8=True)
    assert np.array_equal(_bits(got), _bits(want)) and last8 == last == synth.u8_to_cf32(b)[-1]
    # the format may change between calls: the carried sample is float32
    a, prev = api.polar_plan(b[:2 * 1000], mode, 1.3, in_u8=True)
    c, _ = api.polar_plan(synth.u8_to_cf32(b)[1000:], mode, 1.3, prev=prev)
    assert np.array_equal(_bits(np.concatenate([a, c])), _bits(want))
    # any alignment of the host buffers
    raw = np.zeros(8 * n + 3, np.uint8)
    raw[3:] = synth.u8_to_cf32(b).view(np.uint8)
    from simplefe_amd import lib
    y = np.empty(n, np.float32)
    assert lib.load().sfe_dsp_polar_plan(mode, 1.3, lib.FMT_F32, raw.ctypes.data + 3, n, None, y.ctypes.data_as(lib.fp)) == 0
    assert np.array_equal(_bits(y), _bits(want))
