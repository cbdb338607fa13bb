"""CPU-only tests: the C ABI library loads and exports what include/sfe_dsp.h declares, the
host-side logic (time-law replay, drop-in headers, ring buffer, register DFT) is right, and the
product tree never reaches into the oracle.  No compute call is made without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import build, lib
    build.build_lib()
    return lib.load()


def _declared():
    hdr = open(os.path.join(INC, "sfe_dsp.h")).read()
    return sorted(set(re.findall(r"\b(sfe_dsp_[a-z0-9_]+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol(L):
    from simplefe_amd import lib
    declared = _declared()
    assert len(declared) >= 30
    for s in declared:
        assert hasattr(L, s), s
    assert set(declared) == set(lib.SIGNATURES), "ctypes table and header disagree"
    assert b"gfx950" in L.sfe_dsp_version()


def test_header_cites_reference_interfaces():
    hdr = open(os.path.join(INC, "sfe_dsp.h")).read()
    for cite in ("libdsp/blkconv.cxx:34-75", "libdsp/blkconv.cxx:77-110", "libdsp/resample.cxx:85-153",
                 "libdsp/decimate.cxx:69-129", "libdsp/blkconv.h:40-47"):
        assert cite in hdr, cite


def test_no_gpu_means_loud_failure_not_fallback(L):
    """Without a GPU the create calls fail with SFE_ENODEV; nothing computes on the CPU."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    from simplefe_amd import api, lib
    with pytest.raises(api.SfeError) as e:
        api.Fir(np.ones(4, np.float32))
    assert e.value.code == lib.SFE_ENODEV
    with pytest.raises(api.SfeError):
        api.Rs(np.ones(4, np.float32), 1, 64)


def test_product_tree_never_touches_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py may use oracle/ (as the checker)."""
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, "simplefe_amd")):
        if os.sep + "build" in base:
            continue
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(base, f), errors="replace").read()
                if re.search(r"oracle[./]|liboracle|sfe_oracle|libsferef", txt):
                    bad.append(os.path.join(base, f))
    for base, _, files in os.walk(INC):
        for f in files:
            if re.search(r"liboracle|sfe_oracle|libsferef", open(os.path.join(base, f)).read()):
                bad.append(f)
    assert not bad, bad
    out = subprocess.run(["ldd", os.path.join(ROOT, "simplefe_amd", "libsfe_dsp.so")], capture_output=True, text=True).stdout
    assert "oracle" not in out and "sferef" not in out


def test_product_library_reads_no_environment():
    """the product library takes its switches through the C ABI
    (sfe_dsp_rs_set_algo, sfe_dsp_fir_set_zero_copy_max), never from the environment: no getenv in
    the sources outside #ifdef SFE_DIAG blocks (csrc/diag/*.inc are included under one only: checked too),
    and the built libsfe_dsp.so does not even import it."""
    csrc = os.path.join(ROOT, "simplefe_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if os.path.isdir(os.path.join(csrc, f)):
            assert f == "diag", f
            continue
        depth, diag_at = 0, None          # preprocessor nesting; depth at which an SFE_DIAG block opened
        for ln, line in enumerate(open(os.path.join(ROOT, "simplefe_amd", "csrc", f), errors="replace"), 1):
            st = line.strip()
            if st.startswith(("#if", "#ifdef", "#ifndef")):
                depth += 1
                if diag_at is None and re.match(r"#\s*ifdef\s+SFE_DIAG", st):
                    diag_at = depth
            elif st.startswith("#endif"):
                if diag_at == depth:
                    diag_at = None
                depth -= 1
            elif "getenv" in line and not st.startswith("//") and diag_at is None:
                raise AssertionError(f"{f}:{ln}: getenv outside #ifdef SFE_DIAG: {st}")
            elif re.match(r'#\s*include\s+"diag/', st) and diag_at is None:
                raise AssertionError(f"{f}:{ln}: a diagnostic include outside #ifdef SFE_DIAG: {st}")
    lib = os.path.join(ROOT, "simplefe_amd", "libsfe_dsp.so")
    syms = subprocess.run(["nm", "-D", "--undefined-only", lib], capture_output=True, text=True).stdout
    assert "getenv" not in syms, [l for l in syms.splitlines() if "getenv" in l]


def test_default_fir_kernels_use_no_scratch_and_keep_four_workgroups_per_cu():
    """ADVICE r2 (counted vmcnt waits): what hipcc reported for the kernels of the built library
    (simplefe_amd/build/*.resources.json, written by build.py from -Rpass-analysis=kernel-resource-usage).
    The LDS-DMA kernels of the default path spill nothing; every product FIR and transform-domain
    resampler kernel fits 128 VGPRs (4 workgroups per CU), and none spills more than 8 VGPRs."""
    import json
    from simplefe_amd import build as b
    rj = os.path.join(ROOT, "simplefe_amd", "build", "fir_fft.hip.resources.json")
    if not os.path.exists(rj):
        pytest.skip("library was not built by simplefe_amd/build.py in this tree")
    fir = json.load(open(rj))
    seen_default = 0
    for k, r in fir.items():
        fl = b.fir_kernel_flags(k)
        if not fl:
            continue
        assert r["VGPRs"] <= 128 and r["Occupancy"] >= 4, (k, r)
        assert r["VGPRs Spill"] <= 8, (k, r)
        if fl["DMA"] and not fl["WP"]:
            seen_default += 1
            assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (k, r)
    assert seen_default >= 2          # shared filter and per-channel filters
    pf = json.load(open(os.path.join(ROOT, "simplefe_amd", "build", "poly_fft.hip.resources.json")))
    kernels = {k: r for k, r in pf.items() if "poly_fft256_kernel" in k}
    assert len(kernels) >= 52
    for k, r in kernels.items():
        assert r["VGPRs"] <= 128 and r["Occupancy"] >= 4 and r["VGPRs Spill"] <= 2, (k, r)
    assert kernels and all(r["ScratchSize"] == 0 for k, r in kernels.items() if "<5, 3, 2, false, false" in k)      # the headline shape


# ------------------------------------------------------------------ time-law replay
def _plan_stream(L, U, B, n_total, rate, out_len):
    from simplefe_amd import api, lib
    st = lib.TimeState(0, 0.0, 0)
    ns, pos, mu = [], [], []
    for off in range(0, n_total, B):
        m = min(B, n_total - off)
        p, w = api.rs_plan(st, U, m, out_len, rate)
        ns.append(len(p))
        pos.append(p.astype(np.int64) + off * U)
        mu.append(w)
    return ns, np.concatenate(pos), np.concatenate(mu)


@pytest.mark.parametrize("tag", ["1p77", "5o3", "8", "2p5", "0p77"])
def test_plan_counts_match_reference_vector(L, g4, tag):
    """n_out per process() call as the compiled reference produced them (fixtures G4)."""
    B, U = int(g4["B"]), int(g4["U"])
    ns, pos, mu = _plan_stream(L, U, B, len(g4["x"]), float(g4[f"rate_{tag}"]), 4 * B)
    assert ns == g4[f"n_{tag}"].tolist()
    assert np.all(np.diff(pos) >= 1) and np.all((mu >= 0) & (mu < 1))


@pytest.mark.parametrize("name", ["cfg3", "cfg4", "gen", "gen2"])
@pytest.mark.parametrize("B", [4096, 1000, 1001])
def test_plan_counts_match_baseline_shapes(L, g5, name, B):
    rate = float(g5[f"{name}_rate"])
    ns, pos, mu = _plan_stream(L, int(g5[f"{name}_U"]), B, int(g5["n"]), rate, int(np.ceil(B / rate)) + 2)
    assert ns == g5[f"{name}_n_B{B}"].tolist()
    step = np.float32(rate) * np.float32(int(g5[f"{name}_U"]))
    if float(step) == np.floor(float(step)):
        assert not mu.any()                      # integer-valued step: mu == 0 throughout
        assert np.array_equal(pos, np.arange(len(pos)) * int(step))


def test_plan_reproduces_outputs_with_float64_dots(L, g4, orc):
    """(pos, mu) from the plan + an independent float64 polyphase dot == the reference output
    to float32 rounding: the schedule itself is what the GPU kernel consumes."""
    taps, x, U, B = g4["taps"].astype(np.float64), g4["x"].astype(np.float64), int(g4["U"]), int(g4["B"])
    ns, pos, mu = _plan_stream(L, U, B, len(x), float(g4["rate_1p77"]), 4 * B)

    def s(p):
        n, ph = p // U, p % U
        t = taps[ph::U]
        idx = n - np.arange(len(t))
        ok = (idx >= 0) & (idx < len(x))
        return float(np.dot(t[ok], x[idx[ok]]))
    y = np.array([s(p) * (1.0 - float(m)) + float(m) * s(p + 1) for p, m in zip(pos, mu)])
    assert np.max(np.abs(y - g4["y_1p77"])) < 2e-6


# ------------------------------------------------------------------ C++ host pieces
def _cxx(args, **kw):
    return subprocess.run(args, capture_output=True, text=True, **kw)


def test_ring_buffer_reference_scenarios(tmp_path):
    """gr-simplefe/lib/qa_simplefe.cc:103-166 restated on include/ringbuf.h."""
    exe = str(tmp_path / "rb")
    r = _cxx(["g++", "-O1", "-Wall", "-fsanitize=address,undefined", os.path.join(ROOT, "tests/host/test_ringbuf.cpp"), "-o", exe])
    assert r.returncode == 0, r.stderr
    r = _cxx([exe])
    assert r.returncode == 0 and "ringbuf ok" in r.stdout, r.stdout + r.stderr


def test_ring_buffer_scenarios_hold_on_the_reference_header_too(tmp_path):
    """The same scenario program compiled against the reference's own libdsp/ringbuf.h (in
    place): both classes pass, i.e. they behave alike wherever the reference asserts anything.
    Authoring container only (the reference tree does not travel)."""
    ref = "/root/reference/libdsp"
    if not os.path.exists(os.path.join(ref, "ringbuf.h")):
        pytest.skip("reference tree not present")
    exe = str(tmp_path / "rb_ref")
    r = _cxx(["g++", "-O1", "-w", "-fsanitize=address,undefined", "-DSFE_REF_RINGBUF", "-I" + ref,
              os.path.join(ROOT, "tests/host/test_ringbuf.cpp"), "-o", exe])
    assert r.returncode == 0, r.stderr
    r = _cxx([exe])
    assert r.returncode == 0 and "ringbuf ok" in r.stdout, r.stdout + r.stderr


def test_register_dft16_host_check(tmp_path):
    exe = str(tmp_path / "fft16")
    r = _cxx(["/opt/rocm/bin/hipcc", "-O2", "-x", "hip", "--offload-arch=gfx950",
              os.path.join(ROOT, "tests/host/test_fft16.cpp"), "-o", exe])
    assert r.returncode == 0, r.stderr
    r = _cxx([exe])
    assert r.returncode == 0, r.stdout


def test_dropin_headers_compile_and_link(L, tmp_path):
    """A caller written against the reference's class surface builds against include/ and
    links libsfe_dsp.so (run on the GPU by tests/test_gpu_dropin.py)."""
    exe = str(tmp_path / "dropin")
    libdir = os.path.join(ROOT, "simplefe_amd")
    r = _cxx(["g++", "-O1", "-Wall", os.path.join(ROOT, "tests/host/test_dropin.cpp"), "-o", exe,
              "-L" + libdir, "-lsfe_dsp", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
              "-Wl,--allow-shlib-undefined"])
    assert r.returncode == 0, r.stderr


def test_gr_shaped_blocks_compile_and_link(L, tmp_path):
    """include/gr_sfe/blocks.h against the stand-in runtime header (GNU Radio is not installed)."""
    exe = str(tmp_path / "gr")
    libdir = os.path.join(ROOT, "simplefe_amd")
    r = _cxx(["g++", "-O1", "-Wall", "-std=c++11", os.path.join(ROOT, "tests/host/test_gr_blocks.cpp"), "-o", exe,
              "-L" + libdir, "-lsfe_dsp", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
              "-Wl,--allow-shlib-undefined"])
    assert r.returncode == 0, r.stderr


def test_reference_own_test_program_builds_against_dropin_header(L):
    """libdsp/test/test_blkconv.cxx, unmodified, against include/blkconv.h (oracle/Makefile
    `dropin`); only where /root/reference exists."""
    if not os.path.isdir("/root/reference"):
        pytest.skip("reference tree absent")
    r = _cxx(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "dropin"])
    assert r.returncode == 0, r.stderr
    assert os.path.exists(os.path.join(ROOT, "oracle/_ref/test_blkconv_dropin"))


def test_time_law_closed_form_matches_literal_replay(tmp_path):
    """csrc/timelaw.h: constant-increment runs per float32 binade == the step-by-step recurrence,
    bit for bit, over 1500 random (U, rate, chunk, out_len) cases (tests/host/test_timelaw.cpp)."""
    exe = str(tmp_path / "tl")
    r = _cxx(["g++", "-O2", "-Wall", "-std=c++14", os.path.join(ROOT, "tests/host/test_timelaw.cpp"), "-o", exe])
    assert r.returncode == 0, r.stderr
    r = _cxx([exe])
    assert r.returncode == 0 and "timelaw ok" in r.stdout, r.stdout + r.stderr


def test_split_general_rate_tiles_hold_every_part_span(tmp_path):
    """csrc/segtile.h: a reference call larger than the LDS is dealt to up to 64 workgroups of the direct general-rate kernel,
    each staging the input its outputs reach.  The tile is sized from every part's real span: over blksize 4096 ... 2^20, 7 upsample
    factors, 9 rates, 4 filter lengths (and two whose taps leave the LDS), real and complex, 8 calls and a ragged one with the
    state carried (out_len-exhausted calls included), each launch either refuses or holds every part -- checked against the
    kernel's own tile indexing.  The launcher's rule before it (max_m / split + ceil(rate) + 64 + plen + 2) must overflow on
    complex blksize 393216, U 3, rate 1.0233 (tests/host/test_seg_split.cpp)."""
    exe = str(tmp_path / "ss")
    r = _cxx(["g++", "-O2", "-Wall", "-std=c++14", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
              os.path.join(ROOT, "tests/host/test_seg_split.cpp"), "-o", exe])
    assert r.returncode == 0, r.stderr
    r = _cxx([exe], timeout=600)
    assert r.returncode == 0 and "segsplit ok" in r.stdout, r.stdout + r.stderr
    assert "worst part over by 44 (call 3, part 62)" in r.stdout, r.stdout


def test_bench_gpus_n_without_a_gpu_fails_loudly():
    """`python bench.py --gpus 2` on a host without a GPU: non-zero exit, no JSON line (the round-1
    script printed an n_gpus=1 line for --gpus 8; ADVICE bench.py:125)."""
    import subprocess
    import sys
    if os.path.exists("/dev/kfd"):
        pytest.skip("host has a GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode != 0 and "{" not in r.stdout


def test_product_library_has_no_diagnostic_kernels_or_switches():
    """VERDICT r1 / ADVICE: a product entry point must not be able to return a non-result.  The
    bare access-pattern kernels and the variant / ablation switches exist only under -DSFE_DIAG
    (libsfe_dsp_diag.so, scripts/ only); the product library carries neither the kernels nor the
    environment variable names that used to select them."""
    from simplefe_amd import lib
    blob = open(lib.LIB_PATH, "rb").read()
    for needle in (b"copy_pattern", b"SFE_FIR_VARIANT", b"SFE_FIR_DIAG", b"SFE_FIR_WG_PER_CU", b"SFE_RS_DIAG",
                   b"SFE_MFMA_WG_PER_CU", b"SFE_DEBUG_OCC"):
        assert needle not in blob, needle
    for f in ("simplefe_amd/api.py", "simplefe_amd/lib.py", "bench.py"):
        assert "libsfe_dsp_diag" not in open(os.path.join(ROOT, f)).read(), f
    # __graft_entry__.build() compiles the diagnostic flavour (it must keep building); smoke() never loads it
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "diag" not in entry[entry.index("def smoke"):]


def test_seek_state_equals_the_replayed_recurrence():
    """sfe_dsp_rs_plan_seek (closed form, integer-valued steps) against the literal replay of the
    reference's float32 time law chunk by chunk (sfe_dsp_rs_plan == resample.cxx:119-150): the
    state after n samples must be identical whatever the chunking -- including cuts that leave a
    pending leftover output (position n*U - 1)."""
    from simplefe_amd import api, lib
    L = lib.load()
    for U, S in ((3, 5), (1, 8), (4, 6), (2, 7), (1, 1), (3, 3)):
        rate = float(np.float32(S) / np.float32(U))
        for n in list(range(0, 40)) + [1000, 1001, 4095, 4096, 12345]:
            st = lib.TimeState(0, 0.0, 0)
            left = n
            while left > 0:
                m = min(left, 997)
                api.rs_plan(st, U, m, m * U // S + 8, rate)
                left -= m
            got = lib.TimeState(7, 0.5, 1)
            assert L.sfe_dsp_rs_plan_seek(C.byref(got), U, n, rate) == lib.SFE_OK
            assert (got.pos, got.mu, got.leftover) == (st.pos, st.mu, st.leftover), (U, S, n)
    st = lib.TimeState(0, 0.0, 0)
    assert L.sfe_dsp_rs_plan_seek(C.byref(st), 4, 100, 1.77) == lib.SFE_ESTATE     # no closed form: must be carried


def test_gr_adapters_follow_the_runtime_shared_pointer():
    """GNU Radio 3.7 holds blocks in boost::shared_ptr and connect() takes
    gr::basic_block_sptr.  tests/host/test_gr_sptr.cpp swaps a boost-like template into the
    stand-in runtime and static_asserts that every adapter's sptr is that template, converts to
    basic_block_sptr, inherits virtually from the runtime block types and hides its constructor
    in an _impl class (gr-simplefe/include/simplefe/source_c.h:36-49)."""
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-fsyntax-only", os.path.join(ROOT, "tests/host/test_gr_sptr.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_fir_partition_plan():
    """sfe_dsp_fir_plan (host-only): every tap count gets an overlap that is a multiple of 256 and
    enough partitions to hold the taps; short filters stay one launch with the smallest overlap;
    the cost per output sample (launches / advance) never jumps the way a single 4096-point
    transform's does near 3841 taps."""
    from simplefe_amd import lib
    L = lib.load()
    o, p, a = C.c_int(), C.c_int(), C.c_int()

    def plan(n):
        assert L.sfe_dsp_fir_plan(n, C.byref(o), C.byref(p), C.byref(a)) == lib.SFE_OK
        return o.value, p.value, a.value
    assert plan(1) == (256, 1, 3840) and plan(256) == (256, 1, 3840) and plan(257) == (256, 1, 3840)
    assert plan(258) == (512, 1, 3584) and plan(551)[1] == 1 and plan(2001) == (2048, 1, 2048)
    prev = 0.0
    for n in sorted(list(range(1, 9000, 37)) + [3841, 3842, 4096, 8192, 65536, 245765, 1 << 20]):
        ov, parts, adv = plan(n)
        assert ov % 256 == 0 and 256 <= ov < 4096 and adv == 4096 - ov
        assert (parts == 1 and n <= ov + 1) or (parts > 1 and parts * ov >= n)
        cost = (parts + 0.25 * (parts - 1)) / adv
        single = 1.0 / (4096 - 256 * ((max(n - 1, 1) + 255) // 256)) if n <= 3841 else float("inf")
        assert cost <= single * (1 + 1e-12)
        if n > 1 and n < 9000:
            assert cost >= prev * 0.999          # longer filters never get cheaper
        if n < 9000:
            prev = cost
    assert plan(3841)[1] == 2 and plan(3841)[0] == 2048
    assert L.sfe_dsp_fir_plan(5_000_000, None, None, None) == lib.SFE_ERANGE


def test_work_counter_arithmetic_covers_every_transform_once_and_returns_to_zero():
    """The model of the kernels' draw (csrc/fir_fft.hip, csrc/poly_fft.hip: group g's counter deals runs of
    2^tqs consecutive transforms, ticket c -> ((c >> tqs) * groups + g << tqs) + (c & (2^tqs - 1)); the
    group's last draw -- its share plus one failed draw per workgroup -- puts the counter back to zero):
    every transform is drawn exactly once and every counter ends at zero, whatever the shape."""
    import random

    def run(total, tg, tqs, grid):
        Q, row = 1 << tqs, tg << tqs
        rem = total % row
        last = []
        for g in range(tg):
            mine = (total // row << tqs) + (min(rem - g * Q, Q) if rem > g * Q else 0)
            last.append(mine + (grid - g + tg - 1) // tg - 1)
        ctr, done, alive = [0] * tg, [0] * total, list(range(grid))
        while alive:
            nxt = []
            for b in alive:
                g = b % tg
                c = ctr[g]
                ctr[g] = 0 if c == last[g] else c + 1
                k = (((c >> tqs) * tg + g) << tqs) + (c & (Q - 1))
                if k < total:
                    done[k] += 1
                    nxt.append(b)
            alive = nxt
        assert all(d == 1 for d in done), (total, tg, tqs, grid)
        assert all(c == 0 for c in ctr), (total, tg, tqs, grid)

    rng = random.Random(7)
    for _ in range(1500):
        tg = rng.choice([1, 2, 3, 8])
        grid = rng.randint(tg, 64)
        run(rng.randint(grid + 1, 2000), tg, rng.choice([0, 1, 3, 5]), grid)
    for total in range(9, 200):
        run(total, 8, 3, 8)


def test_bench_notices_an_input_that_lost_its_data():
    """bench.py's parity windows feed the oracle what the device holds, so an input that became zeros would pass them (and the
    FIR runs 10 % faster on it: round 4).  verify_input compares windows of the input with the host generator
    bit for bit; here on CPU tensors: the intact stream passes, a stream with one zeroed stretch fails, derived inputs are
    skipped."""
    import importlib.util
    import torch
    from simplefe_amd import synth
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = 1 << 16

    class Leg:
        pass
    leg = Leg()
    leg.x = torch.from_numpy(np.concatenate([synth.synth_f32(2 * n, synth.SEED, 3), synth.synth_f32(2 * n, synth.SEED, 4)]))
    leg.input_spec = [(0, 2 * n, 3), (2 * n, 2 * n, 4)]
    ctx = {"synth": synth}
    assert bench.verify_input(ctx, leg) is True
    leg.x[2 * n + 2 * n - 4096:] = 0.0                     # the last window of the last region
    assert bench.verify_input(ctx, leg) is False
    leg.input_spec = None
    assert bench.verify_input(ctx, leg) is None


def test_bench_telemetry_never_raises():
    """bench.py --telemetry is best effort: whatever rocm-smi or the device do, the field is a JSON-serialisable dict (here, on a
    host without a GPU, the synchronise fails or rocm-smi has nothing to show)."""
    import importlib.util
    import json
    import torch
    spec = importlib.util.spec_from_file_location("bench_module_t", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    class Leg:
        step = staticmethod(lambda: None)
    got = bench.telemetry({"torch": torch}, Leg(), 40.0)
    assert isinstance(got, dict) and ("error" in got or "reads_while_running" in got)
    json.dumps(got)


def test_time_law_of_the_library_and_of_the_oracle_agree_call_by_call_property(L, orc):
    """Property test (hypothesis): the library's host replay of the reference's float32 time law (sfe_dsp_rs_plan = timelaw.h:
    time_law, what every GPU path places its outputs by) and the oracle's restatement of libdsp/resample.cxx:119-150
    (sfe_oracle.c: timelaw_run, driven without samples by orc_resample_skip_calls) walk the SAME sequence of states: after every
    call the same number of outputs and bit for bit the same (m_pos, m_mu, m_is_leftover) -- for random upsampling factors, call
    lengths, rates from 1 / U upwards (a step of exactly 1 included) and streams of calls of unequal length."""
    from hypothesis import given, settings, strategies as hst
    from simplefe_amd import api, lib

    @settings(max_examples=120, deadline=None)
    @given(U=hst.integers(1, 8), B=hst.integers(1, 700), frac=hst.floats(0.0, 1.0), top=hst.sampled_from([1.0, 1.5, 3.0, 9.0, 40.0]),
           cuts=hst.lists(hst.integers(1, 700), min_size=1, max_size=12))
    def prop(U, B, frac, top, cuts):
        lo = 1.0 / U
        rate = float(np.float32(lo + frac * (max(top, lo) - lo)))
        while float(np.float32(rate)) < lo:                       # the reference refuses rate < 1 / U (resample.cxx:91)
            rate = float(np.nextafter(np.float32(rate), np.float32(np.inf)))
        taps = np.ones(U, np.float32)
        o = orc.Resample(taps, U, 700)
        st = lib.TimeState(0, 0.0, 0)
        for m in [min(c, 700) for c in cuts] + [B]:
            out_len = m * U + 8                                   # a step is >= 1: never the limit
            p, w = api.rs_plan(st, U, m, out_len, rate)
            k = o.skip_calls(1, m, rate)
            assert k == len(p), (U, m, rate)
            pos, mu, left = o.get_time()
            assert (pos, left) == (st.pos, st.leftover) and np.float32(mu).tobytes() == np.float32(st.mu).tobytes(), (U, m, rate, pos, st.pos, mu, st.mu)
            if len(p):
                assert np.all(np.diff(p.astype(np.int64)) >= 1) and np.all((w >= 0) & (w < 1))
    prop()


def test_kernel_source_hash_ignores_comments_and_diagnostic_blocks_and_other_kernels(tmp_path, monkeypatch):
    """simplefe_amd/build.py: csrc_hash -- the stamp a counter pass carries.  A reworded comment, a change inside
    `#ifdef SFE_DIAG` ... `#else` / `#endif`, or a change to ANOTHER kernel's file must not orphan a pass; a change to the
    kernel's own code, or to the product branch of a diagnostic conditional, must."""
    from simplefe_amd import build as b
    monkeypatch.setattr(b, "CSRC", str(tmp_path))

    def write(fir_body, other="int other;\n"):
        (tmp_path / "fir_fft.hip").write_text(fir_body)
        (tmp_path / "fft16.h").write_text("// header\nint f16;\n")
        (tmp_path / "common.h").write_text("int common;\n")
        (tmp_path / "polyphase.hip").write_text(other)
        return b.csrc_hash("fir"), b.csrc_hash("decimate"), b.csrc_hash()

    base = "int a;   // one\n#ifdef SFE_DIAG\nint diag_only;\n#if 1\nint nested;\n#endif\n#else\nint product_branch;\n#endif\nint b;\n"
    h0 = write(base)
    assert write(base.replace("// one", "// another wording"))[0] == h0[0]
    assert write(base.replace("int diag_only;", "int diag_only; int more_diag;").replace("int nested;", "int nested2;")) == h0
    fir, dec, all_ = write(base, other="int other; int changed;\n")
    assert fir == h0[0] and dec != h0[1] and all_ != h0[2]
    assert write(base.replace("int b;", "int b2;"))[0] != h0[0]
    assert write(base.replace("int product_branch;", "int product_branch2;"))[0] != h0[0]
