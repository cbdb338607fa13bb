"""The OFDM modulator's host plan (sfe_dsp_ofdmmod_plan: csrc/ofdmmod_law.h compiled for the host, the reference of the
device's bits) on a machine without a GPU.  Against synth.ofdm_signal, the float64 np.fft synthesiser, at the bar the
receiver's float32 transforms are held to; the promises about bits, literally; the exact case mated with the receiver's;
the round trip through ofdm_plan; every refusal with its message prefix; the build lists; and the law header through a
stand-alone program built with -fsanitize=address,undefined (tests/host/test_ofdmmod_law.cpp)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ofdm_cases as oc
import ofdmmod_cases as mc
from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a, build
    build.build_lib()
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


def frames(api, args, data, lead=3, gap=5, tail=4):
    """The plan's stream of len(data) frames `gap` samples apart behind `lead` samples; (stream, the frames' starts, F)."""
    F = mc.sizes(args)[3]
    nb = len(data)
    starts = lead + np.arange(nb) * (F + gap)
    y = api.ofdmmod_plan(**args, data=data, n_out=lead + nb * (F + gap) + tail, start_base=lead, start_step=F + gap)
    return y, starts, F


# ---- against the float64 synthesiser
@pytest.mark.parametrize("mode", mc.MODES, ids=mc.MODE_IDS)
@pytest.mark.parametrize("name", mc.HOST_NAMES)
def test_the_plan_against_the_float64_synthesiser(api, name, mode):
    """Every kernel size on shapes that use every bin (DC and N / 2 included), and n64 and n4096: each symbol of two frames
    within 1e-5 relative RMS of synth.ofdm_signal's.  Worst seen over the grid: 1.23e-7 (N = 4096, SYMBOLS mode)."""
    _, order, in_mode = mode
    args = mc.shape_args(name, amp=0.5, order=order, in_mode=in_mode)
    Nd, nsym, Ls, F, n = mc.sizes(args)
    assert api.ofdmmod_plan(**args) == (Nd, F, n)
    data = mc.rows(args, 2, 3, pad=1)
    y, starts, _ = frames(api, args, data)
    worst = max(mc.worst_symbol_rms(y[o:o + F], mc.reference_frame(args, data[b]), args) for b, o in enumerate(starts))
    print("ofdmmod plan against float64: %s %s worst symbol rel-RMS %.3e" % (name, mode[0], worst))
    assert worst <= mc.RMS_BAR


# ---- the promises about bits
@pytest.mark.parametrize("name", ["g64", "g128", "g2048", "n512", "n4096"])
def test_the_exact_case_literally(api, name):
    """Every bin a data bin, order 2, amp 1, all bits 0, train all ones: every symbol is exactly 1+0j at its sample cp and
    zero at every other sample -- but for n512, whose prefix is the whole symbol (cp = N), sample 0 is the copy of sample cp."""
    args = mc.exact_args(name)
    Nd, nsym, Ls, F, n = mc.sizes(args)
    y = api.ofdmmod_plan(**args, data=np.zeros((1, n), np.uint8), n_out=F)
    want = np.zeros((nsym, Ls), np.complex64)
    want[:, args["cp"]] = 1.0
    if args["cp"] == args["n_fft"]:
        want[:, 0] = 1.0
    assert (y.reshape(nsym, Ls) == want).all()


@pytest.mark.parametrize("name", ["g64", "g128", "g256", "n512", "n4096"])
def test_the_prefix_is_the_tail_bit_for_bit(api, name):
    args = mc.shape_args(name, amp=0.7)
    Nd, nsym, Ls, F, n = mc.sizes(args)
    N, cp = args["n_fft"], args["cp"]
    y = api.ofdmmod_plan(**args, data=mc.rows(args, 1, 8), n_out=F).reshape(nsym, Ls)
    assert cp > 0 and mc.same(np.ascontiguousarray(y[:, :cp]), np.ascontiguousarray(y[:, N:N + cp]))


@pytest.mark.parametrize("mode", mc.MODES, ids=mc.MODE_IDS)
def test_a_frame_depends_on_its_row_alone_and_the_rest_is_plus_zero(api, mode):
    """The same rows at another burst index, stride and offset give the same words; every sample in no frame has the bit
    pattern of +0."""
    _, order, in_mode = mode
    args = mc.shape_args("g128", amp=0.5, order=order, in_mode=in_mode)
    F = mc.sizes(args)[3]
    data = mc.rows(args, 3, 5)
    y, starts, _ = frames(api, args, data, lead=3, gap=5, tail=4)
    padded = np.concatenate([data[::-1], data[::-1][:, :7]], axis=1)         # reversed order, a longer stride
    z, zstarts, _ = frames(api, args, padded, lead=10, gap=1, tail=0)
    for b in range(3):
        assert mc.same(y[starts[b]:starts[b] + F], z[zstarts[2 - b]:zstarts[2 - b] + F]), b
        one = api.ofdmmod_plan(**args, data=data[b], n_out=F + 9, start_base=9)
        assert mc.same(one[9:], y[starts[b]:starts[b] + F]) and not one[:9].view(np.uint32).any()
    inside = np.zeros(y.size, bool)
    for o in starts:
        inside[o:o + F] = True
    assert not y[~inside].view(np.uint32).any() and (~inside).sum() == 3 + 2 * 5 + 5 + 4


@pytest.mark.parametrize("name", ["g64", "g256", "g2048one", "n4096"])
def test_tx10_is_the_converter_of_the_f32_plan(api, L, name):
    sh = oc.shape(name)
    cp = sh["cp"] + (sh["cp"] & 1)
    place = None
    for in_mode, order in ((mc.BITS, 4), (mc.SYMBOLS, 4)):
        args = mc.shape_args(name, amp=0.6, order=order, in_mode=in_mode, cp=cp)
        F = mc.sizes(args)[3]
        data = mc.rows(args, 2, 11)
        place = dict(n_out=2 * F + 20, start_base=6, start_step=F + 8)
        y = api.ofdmmod_plan(**args, data=data, **place)
        args["out_fmt"] = L.FMT_TX10
        t = api.ofdmmod_plan(**args, data=data, **place)
        assert t.dtype == np.uint8 and t.size == place["n_out"] // 2 * 5 and np.array_equal(t, synth.tx10_pack(y))
    zeros = api.ofdmmod_plan(**args, data=np.zeros((0, 1), np.complex64), n_out=40)
    assert (zeros.reshape(-1, 5) == [0xAA, 0, 0, 0, 0]).all()


# ---- mated with the receiver
@pytest.mark.parametrize("name", ["n64", "n128", "n512", "g2048"])
def test_the_exact_cases_mate(api, L, name):
    """ofdmmod_plan's exact-case stream is the input of ofdm_plan's exact case (advance 0): every Z is exactly 1+0j."""
    args = mc.exact_args(name)
    Nd, nsym, Ls, F, n = mc.sizes(args)
    x, starts, _ = frames(api, args, np.zeros((2, n), np.uint8), lead=5, gap=3, tail=8)
    rx = dict(n_fft=args["n_fft"], cp=args["cp"], advance=0, n_train=1, n_data=args["n_data"], kind=args["kind"], train=args["train"])
    for out_mode in (L.OFDM_OUT_ZF, L.OFDM_OUT_MRC):
        sym, ch, rec, st = api.ofdm_plan(**rx, out_mode=out_mode, x=x, n_bursts=2, start_base=5, start_step=F + 3)
        assert not st.any() and (sym == np.complex64(1.0)).all() and (ch == np.complex64(1.0)).all() and (rec[:, 1] == 1.0).all()


@pytest.mark.parametrize("name", ["n64", "g128", "g512", "g1024", "n4096"])
def test_the_round_trip_returns_the_sent_symbols(api, L, name):
    """ofdm_plan on ofdmmod_plan's noiseless waveform (advance 0, no offset estimate) returns the sent QPSK symbols within
    1e-5 worst error vector; DESIGN.md 4.23 reports 2e-7 for this situation."""
    args = mc.shape_args(name, amp=1.0, order=4)
    Nd, nsym, Ls, F, n = mc.sizes(args)
    data = mc.rows(args, 2, 21)
    x, starts, _ = frames(api, args, data, lead=7, gap=9, tail=0)
    sym, ch, rec, st = api.ofdm_plan(n_fft=args["n_fft"], cp=args["cp"], advance=0, n_train=args["n_train"], n_data=args["n_data"],
                                     kind=args["kind"], train=args["train"], pilot=args["pilot"], pilot_sign=args["pilot_sign"], x=x, n_bursts=2,
                                     start_base=7, start_step=F + 9)
    sent = np.stack([mc.sent_symbols(args, r) for r in data])
    worst = float(np.abs(sym.astype(np.complex128) - sent).max())
    print("ofdmmod -> ofdm round trip: %s worst error vector %.3e" % (name, worst))
    assert not st.any() and worst <= 1e-5


# ---- refusals
def test_every_refusal_of_the_shape_and_its_prefix(api, L):
    lib = L.load()
    good = mc.shape_args("n64", amp=0.5)
    assert api.ofdmmod_plan(**good) == (54, 8 * 80, 81)
    nan, inf = float("nan"), float("inf")

    def broken(table, k, v):
        t = np.array(good[table], copy=True)
        t[k] = v
        return {table: t}

    pil = int(np.flatnonzero(good["kind"] == 2)[0])
    dat = int(np.flatnonzero(good["kind"] == 1)[0])
    nul = int(np.flatnonzero(good["kind"] == 0)[0])
    def sized(n):
        return dict(n_fft=n, kind=np.ones(n, np.uint8), train=np.ones(n, np.complex64), pilot=None, pilot_sign=None)

    bad = [sized(32), sized(8192), sized(96), dict(cp=-1), dict(cp=65), dict(n_train=0), dict(n_train=5), dict(n_data=0),
           dict(n_data=4097, pilot_sign=None), dict(amp=0.0), dict(amp=-1.0), dict(amp=nan), dict(amp=inf), dict(order=3), dict(order=8), dict(in_mode=2),
           dict(in_mode=-1), dict(out_fmt=L.FMT_U8), dict(out_fmt=3), dict(cp=15, out_fmt=L.FMT_TX10), dict(kind=np.zeros(64, np.uint8)),
           broken("kind", 3, 3), dict(kind=np.where(good["kind"] == 1, 0, good["kind"])), broken("train", dat, 0), broken("train", pil, 0),
           broken("train", nul, nan), broken("train", dat, inf), broken("pilot", pil, 0), broken("pilot", nul, nan), dict(pilot=None),
           broken("pilot_sign", 2, 0), broken("pilot_sign", 0, 2)]
    for change in bad:
        with pytest.raises(api.SfeError) as e:
            api.ofdmmod_plan(**{**good, **change})
        assert e.value.code == L.SFE_EINVAL and lib.sfe_dsp_last_error().startswith(b"ofdmmod: "), (change, lib.sfe_dsp_last_error())
        with pytest.raises(api.SfeError) as e:                     # create refuses the same before it looks for a device
            api.OfdmMod(**{**good, **change})
        assert e.value.code == L.SFE_EINVAL and lib.sfe_dsp_last_error().startswith(b"ofdmmod: "), change
    # what is allowed: a zero train value on a null bin, cp = 0 and cp = N, an odd cp in F32
    for change in (broken("train", nul, 0), dict(cp=0), dict(cp=64), dict(cp=15)):
        api.ofdmmod_plan(**{**good, **change})
    assert lib.sfe_dsp_ofdmmod_plan(64, 16, 2, 6, None, None, None, None, 0.5, 4, 0, 0, None, 0, 0, 0, 0, 0, None, None, None, None) == L.SFE_EINVAL
    assert lib.sfe_dsp_last_error().startswith(b"ofdmmod: ")
    with pytest.raises(api.SfeError):
        api.ofdmmod_footprint(100)
    assert api.ofdmmod_footprint(64) == (64, 4096, 512) and api.ofdmmod_footprint(4096) == (256, 4096, 32768)


@pytest.mark.parametrize("fmt", ["f32", "tx10"])
def test_every_refusal_of_the_placement_and_its_prefix(api, L, fmt):
    lib = L.load()
    args = mc.shape_args("n64", amp=0.5, out_fmt=L.FMT_TX10 if fmt == "tx10" else L.FMT_F32)
    F, n = 8 * 80, 81
    data = mc.rows(args, 3, 1)
    good = dict(n_out=3 * F + 8, start_base=2, start_step=F + 2)
    api.ofdmmod_plan(**args, data=data, **good)
    bad = [dict(start_base=-2), dict(start_step=F - 2), dict(start_base=10), dict(n_out=3 * F + 4), dict(n_out=1 << 31)]
    if fmt == "tx10":
        bad += [dict(n_out=3 * F + 9), dict(start_base=3), dict(start_step=F + 3)]
    for change in bad:
        with pytest.raises(api.SfeError) as e:
            api.ofdmmod_plan(**args, data=data, **{**good, **change})
        assert e.value.code == L.SFE_EINVAL and lib.sfe_dsp_last_error().startswith(b"ofdmmod: "), change
        with pytest.raises(api.SfeError):                           # the placement is checked without data too
            api.ofdmmod_plan(**args, n_bursts=3, **{**good, **change})
    with pytest.raises(api.SfeError) as e:
        api.ofdmmod_plan(**args, data=data, n_bursts=1 << 31, **good)
    assert e.value.code == L.SFE_EINVAL
    with pytest.raises(api.SfeError) as e:
        api.ofdmmod_plan(**args, data=data[:, :n - 1], **good)
    assert e.value.code == L.SFE_ERANGE and lib.sfe_dsp_last_error().startswith(b"ofdmmod: ")
    with pytest.raises(api.SfeError) as e:                         # null input with bursts
        api.ofdmmod_plan(**args, data=np.zeros((0, n), np.uint8), n_bursts=1, n_out=F)
    assert e.value.code == L.SFE_EINVAL
    # one burst ignores start_step; an odd one too under TX10; in F32 odd placements are fine
    api.ofdmmod_plan(**args, data=data[:1], n_out=F + 2, start_base=2, start_step=3)
    if fmt == "f32":
        api.ofdmmod_plan(**args, data=data, n_out=3 * F + 9, start_base=3, start_step=F + 3)
    # the process_stream refusals that need no device: no handle, no counter
    k = C.c_size_t(5)
    assert lib.sfe_dsp_ofdmmod_process_stream(None, None, 0, 0, 0, 0, None, 0, C.byref(k), None) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_last_error().startswith(b"ofdmmod_process_stream: ")
    assert lib.sfe_dsp_ofdmmod_destroy(None) == L.SFE_OK


# ---- the build
def test_the_kernel_is_registered_and_touches_no_scratch(api):
    from simplefe_amd import build
    res = json.load(open(os.path.join(build.HERE, "build", "ofdmmod.hip.resources.json")))
    assert len(res) == 14 and all("ofdmmod_kernel<" in k for k in res)       # log2 N = 6 .. 12, F32 and TX10
    for k, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["LDS Size"] <= 32 * 1024, (k, r)
    assert "ofdmmod.hip" in build.EXACT_SOURCES and "api_ofdmmod.hip" in build.HOST_SOURCES and build.SCRATCH_FREE["ofdmmod.hip"]
    assert build.KERNEL_FILES["ofdmmod"] == ("ofdmmod.hip", "ofdmmod.h", "ofdmmod_law.h", "ofdm.h", "common.h")
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    exact = re.search(r"set\(SFE_EXACT_SOURCES ([^)]*)\)", cm).group(1).split()
    assert "ofdmmod.hip" in exact and sorted(exact) == sorted(build.EXACT_SOURCES)
    for f in ("ofdmmod.hip", "api_ofdmmod.hip", "ofdmmod.h", "ofdmmod_law.h"):
        assert os.path.exists(os.path.join(build.CSRC, f))


# ---- the law header under the sanitizers
LAW_CASES = [("g64", 2, mc.BITS, mc.F32, None), ("g128", 4, mc.BITS, mc.F32, None), ("g256", 4, mc.SYMBOLS, mc.F32, None),
             ("g512", 4, mc.BITS, mc.TX10, None), ("g2048one", 2, mc.BITS, mc.F32, None), ("g128p1", 4, mc.SYMBOLS, mc.TX10, 10),
             ("n64", 4, mc.BITS, mc.F32, 0), ("n64", 2, mc.BITS, mc.TX10, 64), ("g1024", 4, mc.BITS, mc.F32, None), ("n4096", 4, mc.BITS, mc.TX10, None)]


def test_the_law_under_the_sanitizers(api, tmp_path):
    """tests/host/test_ofdmmod_law.cpp, built with the host compiler and -fsanitize=address,undefined, runs the law header's
    symbol assembly, transform, frame and wire format from heap blocks of exactly the contract's sizes; what it writes is
    ofdmmod_plan's, byte for byte."""
    exe, fin, fout = str(tmp_path / "ofdmmod_law"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    r = subprocess.run(["g++", "-O1", "-Wall", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests/host/test_ofdmmod_law.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    want = []
    with open(fin, "wb") as f:
        for i, (name, order, in_mode, fmt, cp) in enumerate(LAW_CASES):
            args = mc.shape_args(name, amp=0.37, order=order, in_mode=in_mode, out_fmt=fmt, cp=cp)
            Nd, nsym, Ls, F, n = mc.sizes(args)
            N, amp = args["n_fft"], np.float32(args["amp"])
            data = mc.rows(args, 2, 40 + i)
            kind = args["kind"]
            src = np.full(N, -1, np.int32)
            src[kind == 1] = np.arange(Nd)
            src[kind == 2] = -2

            def table(t, used):
                out = np.zeros((N, 2), np.float32)
                if t is not None:
                    t = np.asarray(t, np.complex64)
                    out[used, 0], out[used, 1] = (amp * t.real)[used], (amp * t.imag)[used]
                return out

            sign = np.ones(args["n_data"], np.float32) if args["pilot_sign"] is None else args["pilot_sign"].astype(np.float32)
            f.write(np.array([N.bit_length() - 1, args["cp"], args["n_train"], args["n_data"], order, in_mode, int(fmt == mc.TX10), 2], np.int32).tobytes())
            f.write(np.array([amp], np.float32).tobytes())
            f.write(src.tobytes() + table(args["train"], kind != 0).tobytes() + table(args["pilot"], kind == 2).tobytes() + sign.tobytes())
            f.write(np.ascontiguousarray(data).tobytes())
            want.append(np.concatenate([api.ofdmmod_plan(**args, data=row, n_out=F).view(np.uint8) for row in data]))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ofdmmod law ok: %d cases" % len(LAW_CASES) in r.stdout, r.stdout + r.stderr
    raw, at = np.fromfile(fout, np.uint8), 0
    for case, w in zip(LAW_CASES, want):
        assert np.array_equal(raw[at:at + w.size], w), case
        at += w.size
    assert at == raw.size
