"""CPU: the owning buffer type every device and pinned-host allocation of the library goes through
(vent_analysis_amd/csrc/devbuf.h, the same header the library includes) over a fake allocator with
a live-block set and a "fail the k-th allocation" switch -- tests/devbuf_check.cpp, a stand-alone
program built with AddressSanitizer and UBSan.  It checks reserve's contract (allocates on first
use, nothing when the held size suffices, free-then-allocate on a grow, one element for n == 0,
empty after a failed allocation), that nothing is freed twice, the moves (vh_pipe::Slot lives in a
std::vector), and that the N4 lattice group (three buffers and the stride the kernels index them
with) names no stride over a missing buffer, and leaks nothing, whichever allocation fails."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "vent_analysis_amd", "csrc")
CHECK = os.path.join(HERE, "devbuf_check.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_devbuf_contract_under_sanitizers(tmp_path):
    exe = str(tmp_path / "chk")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, CHECK, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "devbuf ok" in r.stdout and " 0 live" in r.stdout, r.stdout + r.stderr
