"""CPU: the host-to-host pipe's host logic (vent_analysis_amd/csrc/pipe_host.h, the same header
pipe.hip includes) -- tests/pipe_host_check.cpp, a stand-alone program built once with
AddressSanitizer and UBSan and once with ThreadSanitizer.  The range splitter's ranges are disjoint,
ordered, aligned and cover the input; par_pack_mask / par_unpack_maps / par_memcpy / par_touch agree
with bytewise references on both sides of their task sizes; the page plan of a caller range adds up
and consecutive chunks share no body page; the pin budget never passes its cap under eight threads;
the chunk ticket orders three slot threads and its abort wakes every waiter."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "vent_analysis_amd", "csrc")
CHECK = os.path.join(HERE, "pipe_host_check.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitize", [["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                                      ["-fsanitize=thread"]], ids=["asan_ubsan", "tsan"])
def test_pipe_host_logic_under_sanitizers(tmp_path, sanitize):
    exe = str(tmp_path / "chk")
    subprocess.run(["g++", "-std=c++17", "-pthread", "-O2", "-g"] + sanitize +
                   ["-I", CSRC, CHECK, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pipe host ok" in r.stdout, r.stdout + r.stderr
