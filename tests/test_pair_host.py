"""The pair-saturation arithmetic behind every kernel (fast-dnn_amd/csrc/fdnn_pair.hpp: the correction sat16(p) - p, the
dot-product screen, the two entry decoders, the accumulator slot of a node, the entry cursor), checked on the host alone: the
stand-alone checker tests/host/pair_check.cpp states the cases; it is built with the address and undefined-behaviour
sanitizers and run as a child process.  CPU only.  The kernels' use of it: tests/test_gpu_sat_lone_frame.py."""
import os
import subprocess

from conftest import ROOT


def test_pair_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pair_check")
    src = os.path.join(ROOT, "tests", "host", "pair_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "pair ok" in run.stdout
