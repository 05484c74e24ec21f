"""CPU: the host side of the fine registration (vent_analysis_amd/csrc/register_maps_host.h, the same
header the library includes) -- tests/register_maps_check.cpp, a stand-alone program built with
AddressSanitizer and UBSan: the candidate list of one axis against the formula, the pick against a
brute-force search over tied and NaN scores, and the refusals of both."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "vent_analysis_amd", "csrc")
CHECK = os.path.join(HERE, "register_maps_check.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_candidates_and_pick_under_sanitizers(tmp_path):
    exe = str(tmp_path / "chk")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, CHECK, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "register maps host ok" in r.stdout, r.stdout + r.stderr
