"""The drop-in C++ class surface on the GPU: the reference's own test program and a caller
written like the reference's drivers, both linked against libsfe_dsp.so.  `-m gpu`."""
import os
import subprocess

import numpy as np
import pytest

import stream_checks as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "simplefe_amd")


@pytest.fixture(scope="module")
def dropin_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dropin") / "test_dropin")
    r = subprocess.run(["g++", "-O1", os.path.join(ROOT, "tests/host/test_dropin.cpp"), "-o", exe,
                        "-L" + LIBDIR, "-lsfe_dsp", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib",
                        "-Wl,--allow-shlib-undefined"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_reference_test_blkconv_program_unmodified(g1):
    """libdsp/test/test_blkconv.cxx compiled from the reference tree against include/blkconv.h
    (oracle/Makefile `dropin`), run here: it prints blksize and 2 x 28 values with %.2f."""
    exe = os.path.join(ROOT, "oracle/_ref/test_blkconv_dropin")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/test_blkconv_dropin not prebuilt")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert lines[0].strip() == "blksize = 28"
    vals = [l.strip() for l in lines[1:] if l.strip()]
    want = ["%.2f" % v for v in list(g1["out1"]) + list(g1["out2"])]
    assert [v.lstrip("-") for v in vals] == want       # "-0.00" and "0.00" print alike in effect


def test_reference_test_program_built_by_the_committed_cmake_target(g1):
    """The same program built through CMakeLists.txt's `Libdsp` target by a scratch project whose only
    source is the reference's test_blkconv.cxx (tests/test_cmake_dropin.py builds it under
    oracle/_ref/cmake_dropin/), linked to the libsfe_dsp.so CMake built with hipcc: same known answer."""
    build = os.path.join(ROOT, "oracle/_ref/cmake_dropin/build")
    exe = os.path.join(build, "test_blkconv")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/cmake_dropin not prebuilt (tests/test_cmake_dropin.py)")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(build, "sfe_dsp") + ":" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert lines[0].strip() == "blksize = 28"
    vals = [l.strip() for l in lines[1:] if l.strip()]
    want = ["%.2f" % v for v in list(g1["out1"]) + list(g1["out2"])]
    assert [v.lstrip("-") for v in vals] == want
    maps = subprocess.run(["ldd", exe], capture_output=True, text=True, env=env).stdout
    assert "cmake_dropin/build/sfe_dsp/libsfe_dsp.so" in maps, maps      # the CMake-built library, not the in-tree one


def test_reference_test_program_prints_the_same_either_way():
    """test_blkconv.cxx linked the reference's way (its own blkconv.cxx + ROCm's libhipfftw for
    the FFTW calls) and linked to the drop-in: the two programs print the same lines."""
    a = os.path.join(ROOT, "oracle/_ref/test_blkconv_reference")
    b = os.path.join(ROOT, "oracle/_ref/test_blkconv_dropin")
    if not (os.path.exists(a) and os.path.exists(b)):
        pytest.skip("oracle/_ref test programs not prebuilt")
    ra = subprocess.run([a], capture_output=True, text=True, timeout=120)
    rb = subprocess.run([b], capture_output=True, text=True, timeout=120)
    assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr, rb.stderr)
    la = [l.strip().replace("-0.00", "0.00") for l in ra.stdout.split("\n") if l.strip()]
    lb = [l.strip().replace("-0.00", "0.00") for l in rb.stdout.split("\n") if l.strip()]
    assert len(la) == 57 and la == lb


def test_cxx_blkconv_class(dropin_exe, g1):
    r = subprocess.run([dropin_exe, "blkconv"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split()
    assert lines[:3] == ["blksize", "=", "28"]
    v = np.array([float(t) for t in lines[3:]], dtype=np.float64)
    assert np.allclose(v[:28], g1["out1"], atol=2e-6) and np.allclose(v[28:], g1["out2"], atol=2e-6)


@pytest.mark.parametrize("cls", ["resample", "decimate"])
def test_cxx_resampler_classes_bit_exact(dropin_exe, g4, cls, tmp_path):
    """The C++ classes through the driver loop of test_decimate.py:22-25, rate 1.77."""
    g4["taps"].astype(np.float32).tofile(tmp_path / "taps.f32")
    g4["x"].astype(np.float32).tofile(tmp_path / "x.f32")
    B, U = int(g4["B"]), int(g4["U"])
    r = subprocess.run([dropin_exe, "rs", cls, str(tmp_path / "taps.f32"), str(tmp_path / "x.f32"), str(U), str(B),
                        str(4 * B), repr(float(g4["rate_1p77"])), str(tmp_path / "y.f32")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert [int(t) for t in r.stdout.split()] == g4["n_1p77"].tolist()
    assert np.array_equal(np.fromfile(tmp_path / "y.f32", dtype=np.float32), g4["y_1p77"])


# ----------------------------------------------------- GNU-Radio-shaped adapters (N1)
@pytest.fixture(scope="module")
def gr_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gr") / "test_gr_blocks")
    r = subprocess.run(["g++", "-O1", "-std=c++11", os.path.join(ROOT, "tests/host/test_gr_blocks.cpp"), "-o", exe,
                        "-L" + LIBDIR, "-lsfe_dsp", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib",
                        "-Wl,--allow-shlib-undefined"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run_gr(gr_exe, tmp_path, kind, taps, x_il, *extra):
    taps.astype(np.float32).tofile(tmp_path / "t.f32")
    x_il.astype(np.float32).tofile(tmp_path / "x.f32")
    r = subprocess.run([gr_exe, kind, str(tmp_path / "t.f32"), str(tmp_path / "x.f32"), str(tmp_path / "y.f32"),
                        *[str(e) for e in extra]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(tmp_path / "y.f32", dtype=np.float32)


def test_gr_fir_bank_over_device_blocks(gr_exe, tmp_path):
    """fir_bank_ccf_sync: 6 channels on 6 ports, cut into 1, 2 and 4 blocks (all on device 0 here; on an
    8-GPU node the same list names 8 devices), scheduler-sized work() calls incl. one longer than the block's
    staging: every port's stream is its own convolution, and the cut changes no bit."""
    from simplefe_amd import synth
    taps = synth.taps_cfg2()
    nch, n = 6, 30000
    x = np.stack([synth.synth_cf32(n, ch=20 + c) for c in range(nch)])
    outs = [_run_gr(gr_exe, tmp_path, "bank", taps, x, nch, nblk).reshape(nch, 2 * n) for nblk in (1, 2, 4)]
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    for c in range(nch):
        for part in (0, 1):
            ref = np.convolve(x[c, part::2].astype(np.float64), taps.astype(np.float64))[:n]
            assert synth.rel_rms(outs[0][c, part::2], ref) <= 1e-5, c


def test_gr_fir_blocks_batched_and_sync(gr_exe, tmp_path):
    """general_work() / work() called with scheduler-sized item counts (4096, 1000, 8191, 37, 16384):
    the batched block (fir_ccf: pinned batches of 8192 items, four in flight) and the one-round-trip
    block (fir_ccf_sync) both equal one streaming convolution; item k out belongs to item k in
    (nothing is delayed or dropped, the stream end is drained by input-less calls)."""
    from simplefe_amd import synth
    taps = synth.taps_cfg2()
    n = 60000
    x = synth.synth_cf32(n)
    for kind in ("fir", "fir_sync"):
        y = _run_gr(gr_exe, tmp_path, kind, taps, x)
        assert len(y) == 2 * n
        for part in (0, 1):
            ref = np.convolve(x[part::2].astype(np.float64), taps.astype(np.float64))[:n]
            assert synth.rel_rms(y[part::2], ref) <= 1e-5, kind
    xr = synth.synth_f32(n, ch=4)
    y = _run_gr(gr_exe, tmp_path, "fir_f", taps, xr)
    assert synth.rel_rms(y, np.convolve(xr.astype(np.float64), taps.astype(np.float64))[:n]) <= 1e-5


def test_gr_fir_batching_is_5x_the_round_trip_per_call_and_bit_exact(gr_exe, tmp_path):
    """at 4096-item calls the batched block moves >= 5x the items per second of
    one synchronous H2D -> kernel -> D2H round trip per call, and its output is bit for bit what
    the bulk device call produces for the same 262144-item batches."""
    from simplefe_amd import api, lib, synth
    taps = synth.taps_cfg2()
    n = 1 << 23
    x = synth.synth_cf32(n, ch=2)
    taps.astype(np.float32).tofile(tmp_path / "t.f32")
    x.tofile(tmp_path / "x.f32")
    r = subprocess.run([gr_exe, "rate", str(tmp_path / "t.f32"), str(tmp_path / "x.f32"), str(tmp_path / "y.f32")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    batched, sync = (float(v) for v in r.stdout.split()[:2])
    print(f"fir_ccf at 4096-item calls: batched {batched / 1e6:.0f} MS/s, one round trip per call {sync / 1e6:.0f} MS/s")
    assert batched >= 5.0 * sync, (batched, sync)
    y = np.fromfile(tmp_path / "y.f32", dtype=np.float32)
    f = api.Fir(taps, data_complex=True)
    B = 1 << 18
    for off in range(0, n, B):
        got = sc.run_fir(api, f, x[2 * off: 2 * (off + B)])[0]
        assert np.array_equal(got, y[2 * off: 2 * (off + B)]), off


def test_gr_decimate_and_resampler_blocks_bit_exact(gr_exe, tmp_path, g5, orc):
    """sync_decimator by 8 and rational resampler 3/5 over cf32, against the oracle's real
    passes: integer-valued steps, so the scheduler's chunking does not show (bit-exact)."""
    from simplefe_amd import synth
    n = 40000
    x = synth.synth_cf32(n)
    y = _run_gr(gr_exe, tmp_path, "decimate", g5["cfg4_taps"], x, 8)
    for part in (0, 1):
        ref, _ = orc.Decimate(g5["cfg4_taps"], 1, 4096).stream(x[part::2], 8.0)
        got = y[part::2]
        sc.check_total(len(got), len(ref), n, 1, 8.0)
        assert np.array_equal(got, ref)
    y = _run_gr(gr_exe, tmp_path, "resample", g5["cfg3_taps"], x, 5, 3)
    for part in (0, 1):
        ref, _ = orc.Resample(g5["cfg3_taps"], 3, 4096).stream(x[part::2], 5.0 / 3.0)
        got = y[part::2]
        sc.check_total(len(got), len(ref), n, 3, 5.0 / 3.0)
        assert np.array_equal(got, ref)


def test_gr_float_item_blocks_bit_exact(gr_exe, tmp_path, g5, orc):
    """The float-item twins (decimate_fff, rational_resampler_fff: the reference's classes are
    real-valued, its source_f / sink_f blocks carry float items) against the oracle, bit-exact."""
    from simplefe_amd import synth
    n = 50000
    x = synth.synth_f32(n, ch=9)
    y = _run_gr(gr_exe, tmp_path, "decimate_f", g5["cfg4_taps"], x, 8)
    ref, _ = orc.Decimate(g5["cfg4_taps"], 1, 4096).stream(x, 8.0)
    sc.check_total(len(y), len(ref), n, 1, 8.0)
    assert np.array_equal(y, ref)
    y = _run_gr(gr_exe, tmp_path, "resample_f", g5["cfg3_taps"], x, 5, 3)
    ref, _ = orc.Resample(g5["cfg3_taps"], 3, 4096).stream(x, 5.0 / 3.0)
    sc.check_total(len(y), len(ref), n, 3, 5.0 / 3.0)
    assert np.array_equal(y, ref)


def test_gr_wire_format_blocks(gr_exe, tmp_path, orc):
    """The FIR blocks that speak gr-simplefe's wire formats (include/gr_sfe/blocks.h: rx_fir_bc, fir_tx_cb,
    rx_fir_tx_bb): u8 (I,Q) pairs in as source_c receives them (lib/source_c_impl.cc:121-132), 10-bit packed
    bytes out as sink_c sends them (lib/sink_c_impl.cc:118-144), driven with scheduler-sized calls.
    rx: within the bar of the oracle's converter -> filter; tx: the oracle's packing of the filter's own float
    output, byte for byte except codes on a quantiser step (<= 1 LSB); whole 5-byte groups only."""
    from simplefe_amd import api, lib, synth
    taps = synth.taps_cfg2()
    n = 100003                                        # odd: the last sample forms no group
    raw = np.random.default_rng(11).integers(0, 256, size=2 * n, dtype=np.uint8)
    taps.astype(np.float32).tofile(tmp_path / "t.f32")
    raw.tofile(tmp_path / "x.u8")

    def run(kind, xfile):
        r = subprocess.run([gr_exe, kind, str(tmp_path / "t.f32"), str(tmp_path / xfile), str(tmp_path / "y.bin")],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.fromfile(tmp_path / "y.bin", dtype=np.uint8)

    xf = orc.rx_u8_to_cf32(raw)                       # the receive converter, host twin
    ref = np.empty(2 * n, np.float32)
    for part in (0, 1):
        ref[part::2] = orc.Blkconv(taps, 4096).stream(np.ascontiguousarray(xf[part::2]))
    # receive: bytes in, gr_complex out
    y = run("rx_fir", "x.u8").view(np.float32)
    assert len(y) == 2 * n
    for part in (0, 1):
        assert synth.rel_rms(y[part::2], ref[part::2]) <= 1e-5
    # transmit: gr_complex in, 10-bit bytes out
    (0.6 * xf).astype(np.float32).tofile(tmp_path / "x.f32")
    got = run("fir_tx", "x.f32")
    want = orc.tx_f32_to_10bit((0.6 * ref).astype(np.float32))       # linear filter: 0.6 x -> 0.6 y, to float rounding
    assert len(got) == (n // 2) * 5 == len(want)
    dv = np.abs(_unpack10(got) - _unpack10(want))
    assert dv.max() <= 1 and np.count_nonzero(dv) <= 0.004 * len(dv)
    # wire to wire: the source_c -> FIR -> sink_c flowgraph as one block
    got = run("rx_fir_tx", "x.u8")
    want = orc.tx_f32_to_10bit(ref)
    assert len(got) == (n // 2) * 5
    dv = np.abs(_unpack10(got) - _unpack10(want))
    assert dv.max() <= 1 and np.count_nonzero(dv) <= 0.004 * len(dv)


# ------------------------------------------ bpsk pipeline end to end on the GPU path (N3)
def _bpsk_stream(n_blocks, blk):
    """The process thread's symbol generator of examples/bpsk_gpu/bpsk_gpu.cpp, in Python."""
    sps, amp = 10, np.float32(.85) / np.float32(1.35)
    state, n_phase, out = 12345, 0, []
    for _ in range(n_blocks):
        buf = []
        if n_phase > 0:
            for _i in range(n_phase, sps):
                if len(buf) < blk:
                    buf.append(0.0)
            n_phase = 0
        while len(buf) < blk:
            state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
            word = state >> 1
            for j in range(31):
                if len(buf) >= blk:
                    break
                buf.append(-amp if (word >> j) & 1 else amp)
                n_phase = 1
                while n_phase < sps and len(buf) < blk:
                    buf.append(0.0)
                    n_phase += 1
                if n_phase == sps:
                    n_phase = 0
        out.extend(buf)
    return np.array(out, dtype=np.float32)


def _unpack10(b):
    b = b.reshape(-1, 5).astype(np.int32)
    hi = b[:, 0]
    return np.stack([((hi >> (2 * k)) & 3) << 8 | b[:, 1 + k] for k in range(4)], axis=1).reshape(-1)


def test_bpsk_pipeline_end_to_end(tmp_path, orc, g1):
    """examples/bpsk/bpsk.cxx:104-174 on the GPU path: process thread (drop-in blkconv + ring_buffer)
    and a consumer thread doing the converting read (10-bit packing) -- against the same chain
    built from the oracle.  Byte-exact except where a sample sits within float rounding of a
    quantiser step (|difference| <= 1 LSB there)."""
    exe = str(tmp_path / "bpsk_gpu")
    r = subprocess.run(["g++", "-O1", "-pthread", os.path.join(ROOT, "examples/bpsk_gpu/bpsk_gpu.cpp"), "-o", exe,
                        "-L" + LIBDIR, "-lsfe_dsp", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib",
                        "-Wl,--allow-shlib-undefined"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    taps, fft_len, n_blocks = g1["g2_taps"], 2048, 40
    taps.astype(np.float32).tofile(tmp_path / "taps.f32")
    r = subprocess.run([exe, str(n_blocks), str(tmp_path / "tx.bin"), str(fft_len), str(tmp_path / "taps.f32")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(tmp_path / "tx.bin", dtype=np.uint8)
    blk = fft_len + 1 - len(taps)
    x = _bpsk_stream(n_blocks, blk)
    y = orc.Blkconv(taps, fft_len).stream(x)
    n_xfer = len(y) // 2048
    assert len(got) == n_xfer * 2560 and n_xfer > 30
    want = orc.tx_f32_to_10bit(y[: n_xfer * 2048])
    dv = np.abs(_unpack10(got) - _unpack10(want))
    assert dv.max() <= 1 and np.count_nonzero(dv) <= 0.002 * len(dv)


@pytest.mark.gpu
def test_pydsp_module_name_resolves_to_the_gpu_classes(g4):
    """`from pydsp import *` as libdsp/test/test_decimate.py:8, with simplefe_amd/compat on the path:
    the script's loop (test_decimate.py:17-25), checked against the compiled reference's outputs."""
    import importlib
    import sys
    compat = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simplefe_amd", "compat")
    sys.path.insert(0, compat)
    try:
        pydsp = importlib.import_module("pydsp")
    finally:
        sys.path.remove(compat)
    assert set(pydsp.__all__) >= {"resample", "decimate"}
    N, B = 1024, 128
    x0 = g4["x"][:N]
    dec = pydsp.decimate(g4["taps"].tolist(), 4, B)
    y = []
    for b in range(N // B):
        Ny, y0 = dec.process(x0[b * B:(b + 1) * B], 4 * B, float(g4["rate_1p77"]))
        y += y0[0:Ny].tolist()
    assert np.array_equal(np.array(y, dtype=np.float32), g4["y_1p77"][:len(y)]) and len(y) == int(np.sum(g4["n_1p77"]))
