"""What a resample / decimate process_stream call works out before it launches (csrc/rs_plan.h), on the host: the header is
plain C++ and includes nothing from HIP, so a stand-alone program (tests/host/test_rs_plan.cpp) compiles it alone with the
host compiler under -fsanitize=address,undefined and holds the general-rate planner, its run memo (the un-memoised branch in
mid-launch included), the tile-span walk, the host expansion and the integer-step closed form to the literal time_law.
Then the build's bookkeeping.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simplefe_amd", "csrc")


def test_the_planner_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "rs_plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests/host/test_rs_plan.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rs plan ok: " in r.stdout, r.stdout + r.stderr
    print(r.stdout.strip())


def test_the_header_is_host_code_without_hip():
    """rs_plan.h is outside the kernel-source hash and includes no HIP and nothing of the library's but the two host-only
    headers it builds on; host.h includes it, so api_rs.hip sees it."""
    from simplefe_amd import build
    assert "rs_plan.h" in build.HOST_SOURCES
    text = open(os.path.join(CSRC, "rs_plan.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["math.h", "stdint.h", "string.h", "unordered_map", "vector",
                                                                "segtile.h", "timelaw.h"]
    assert "hip" not in re.sub(r"//.*", "", text).lower()
    assert '#include "rs_plan.h"' in open(os.path.join(CSRC, "host.h")).read()


def test_the_integer_step_test_is_written_once():
    """The integral-and-below-1e6 test of a step stands in rs_plan.h alone; api_rs.hip asks the helpers."""
    rs = open(os.path.join(CSRC, "api_rs.hip")).read()
    assert "1.0e6f" not in rs and "16777216" not in rs
    assert rs.count("rs_int_step_law(") == 2 and rs.count("rs_step_is_integer(") == 1
    assert open(os.path.join(CSRC, "rs_plan.h")).read().count("1.0e6f") == 1
