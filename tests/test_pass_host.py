"""What a scoring pass hands each of its chunks (fast-dnn_amd/csrc/fdnn_pass.hpp: the pointers and counts of every named
constructor's chunks, how the chunks' results tile the caller's arrays, and the chunk arithmetic against recorded values),
checked on the host alone: the stand-alone checker tests/host/pass_check.cpp states the cases; it is built with the address
and undefined-behaviour sanitizers and run as a child process.  CPU only."""
import os
import subprocess

from conftest import ROOT


def test_pass_chunks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pass_check")
    src = os.path.join(ROOT, "tests", "host", "pass_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "pass ok" in run.stdout
