"""What a FIR handle works out before it uploads or launches (csrc/fir_plan.h), on the host: the header is plain C++ and
includes nothing from HIP, so a stand-alone program (tests/host/test_fir_plan.cpp) compiles it alone with the host compiler
under -fsanitize=address,undefined and holds the spectrum tables to a direct long-double DFT at the index the kernel reads,
the twiddle bases to their definition, the partition planner to its laws and the variant key's size class to log2.
Then the build's bookkeeping, and the rules that the refactoring left with one definition each.  No GPU."""
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simplefe_amd", "csrc")


def _code(name):
    """A file of csrc without its // comments."""
    return re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())


def test_the_tables_and_the_planner_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "fir_plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests/host/test_fir_plan.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fir plan ok: " in r.stdout, r.stdout + r.stderr
    print(r.stdout.strip())


def test_the_header_is_host_code_without_hip():
    """fir_plan.h is outside the kernel-source hash and includes no HIP and nothing of the library's; host.h includes it, so
    api_fir.hip and api_rs.hip see it."""
    from simplefe_amd import build
    assert "fir_plan.h" in build.HOST_SOURCES
    text = open(os.path.join(CSRC, "fir_plan.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["math.h", "stddef.h", "utility", "vector"]
    assert "hip" not in _code("fir_plan.h").lower()
    assert '#include "fir_plan.h"' in open(os.path.join(CSRC, "host.h")).read()


def test_the_single_transform_overlap_is_written_once():
    """The rows-of-256 rule stands in fir_plan.h alone: the planner, create's fallback and the TX10 re-plan ask it."""
    src = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip"))}
    rule = "+ 255) / 256) * 256"           # (the bare ceiling "+ 255) / 256" also sizes many a launch grid)
    assert [(p, t.count(rule)) for p, t in sorted(src.items()) if rule in t] == [("fir_plan.h", 1)]
    assert src["fir_plan.h"].count("fir_single_overlap(") == 3 and src["api_fir.hip"].count("fir_single_overlap(") == 1
    assert src["api_fir.hip"].count("fir_history_len(") == 1


def test_the_resampler_builds_tables_not_a_fir_handle():
    """api_rs.hip names neither the FIR's create nor its handle; the create is api_fir.hip's own."""
    rs = open(os.path.join(CSRC, "api_rs.hip")).read()
    assert "fir_create_impl" not in rs and not re.search(r"\bFir\b", rs)
    assert "fir_create_impl" not in open(os.path.join(CSRC, "host.h")).read()
    assert "static int fir_create_impl(" in open(os.path.join(CSRC, "api_fir.hip")).read()


def test_the_history_epilogue_and_load_history_are_written_once():
    """The carry-over kernel is launched from two places in the host code: the epilogue of a call (carry_history) and
    load_history, both block.h's; the two handles and the class-compatible host path of the resampler ask them."""
    host = [os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "api*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) if
            os.path.basename(p) != "common.h"]
    assert {p: _code(p).count("launch_history_update(") for p in host if "launch_history_update(" in _code(p)} == {"block.h": 2}
    assert _code("api_fir.hip").count("carry_history(") == 1 and _code("api_rs.hip").count("carry_history(") == 2
    for name, cast in (("api_fir.hip", "as_fir"), ("api_rs.hip", "as_rs")):
        who = name[4:-4]
        assert 'return load_history("%s_load_history", %s(h), d_prev, n_prev, stride, (hipStream_t)stream);' % (who, cast) in _code(name)


def test_the_two_handles_take_their_byte_ranges_from_span_bytes():
    """No range of the FIR or the resampler is multiplied out by hand any more: the three entry points go through the
    channel family of call_checks.h."""
    for name in ("api_fir.hip", "api_rs.hip"):
        code = _code(name)
        assert "n_channels - 1)" not in code and "ranges_overlap(" not in code and "uintptr_t" not in code, name
    assert _code("api_fir.hip").count("check_channels(") == 1 and _code("api_fir.hip").count("fir_check_buffers(") == 3
    assert _code("api_rs.hip").count("check_channels(") == 1
