"""Which kernel a layer launches (fast-dnn_amd/csrc/fdnn_select.hpp: layer 0's kind, an int8 layer's form and tiles, chained
hidden layers, the fused soft-max), checked on the host alone: the stand-alone checker tests/host/select_check.cpp holds the
selection's recorded table (tests/host/select_table.txt), the agreement of the "will it chain / fuse" questions with the pass
planner, and the frame-tile argument of the dispatch ledger's exclusions; it is built with the address and
undefined-behaviour sanitizers and run as a child process.  CPU only."""
import os
import subprocess

from conftest import ROOT


def test_kernel_selection_under_sanitizers(tmp_path):
    exe = str(tmp_path / "select_check")
    src = os.path.join(ROOT, "tests", "host", "select_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "host", "select_table.txt")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "select ok" in run.stdout
