"""The argument checks every process_stream makes before it launches anything (csrc/call_checks.h), on the host: the header
is plain C++ and includes nothing from HIP, so a stand-alone program (tests/host/test_call_checks.cpp) compiles it alone
with the host compiler under -fsanitize=address,undefined and asserts the return code and the whole message of every
rule at its boundary values -- span_bytes, the overlap tests, the starts and placement rules, the one check of each
family (rows, windows, frames, streams, channels) with every entry point's own words, and the byte ranges of combine, corr, mvdr
and eig at strides that would wrap them.  Then the build's bookkeeping.
No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simplefe_amd", "csrc")


def test_the_call_checks_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "call_checks")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests/host/test_call_checks.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "call checks ok: " in r.stdout, r.stdout + r.stderr


def test_the_header_is_host_code_without_hip():
    """call_checks.h is outside the kernel-source hash, includes no HIP and nothing of the library's but the public header;
    block.h includes it, so every block sees the checks it saw before."""
    import re
    from simplefe_amd import build
    assert "call_checks.h" in build.HOST_SOURCES
    text = open(os.path.join(CSRC, "call_checks.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["stddef.h", "stdint.h", "initializer_list", "../../include/sfe_dsp.h"]
    assert "hip" not in re.sub(r"//.*", "", text).lower()
    assert '#include "call_checks.h"' in open(os.path.join(CSRC, "block.h")).read()


def test_each_rule_is_written_once():
    """The starts rule, the placement rule, the pairwise test of the outputs and the refusal of a wrapped byte range each have
    one definition in csrc; the in_stride sentence that names the streams has two there, windows and streams, and a third in
    corr, which keeps its own sequence of rules."""
    import glob
    src = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip"))}
    for words, count, also in (("must stay within +-(2^63 - 2^33)", 1, []), ("frames must not overlap", 1, []),
                               ("the output ranges overlap one another", 1, []), ("the strides take a byte range to 2^62", 1, []),
                               ("in_stride %zu < n_in %zu with %d streams", 2, ["api_corr.hip"])):
        assert sorted(p for p, t in src.items() if words in t) == sorted(["call_checks.h"] + also), words
        assert src["call_checks.h"].count(words) == count and all(src[p].count(words) == 1 for p in also), words
