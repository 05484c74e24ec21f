"""CPU: the state of a resident batch (vent_analysis_amd/csrc/batch_state.h, the same header the
library includes) -- tests/batch_state_check.cpp, a stand-alone program built with AddressSanitizer
and UBSan.  From a fresh state every guard raises VH_ERR_ARG with its message; from the state in
which everything is set each transition of the table in DESIGN.md section 3 changes exactly the
members it lists; ran and forgot_run clear the same derived set; the N4 source is none after
forgot_run and the one given after ran."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "vent_analysis_amd", "csrc")
CHECK = os.path.join(HERE, "batch_state_check.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_batch_state_table_under_sanitizers(tmp_path):
    exe = str(tmp_path / "chk")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, CHECK, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "batch state ok" in r.stdout, r.stdout + r.stderr
