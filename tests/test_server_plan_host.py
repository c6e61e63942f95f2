"""What a batch of the scoring loop contains (fast-dnn_amd/csrc/fdnn_server_plan.hpp: which requests share it, each
piece's rows and pointers, the staged raw frames and segment of a raw piece), checked on the host alone: the stand-alone
checker tests/host/server_plan_check.cpp states the cases; it is built with the address and undefined-behaviour sanitizers
and run as a child process.  CPU only."""
import os
import subprocess

from conftest import ROOT


def test_batch_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "server_plan_check")
    src = os.path.join(ROOT, "tests", "host", "server_plan_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "server plan ok" in run.stdout
