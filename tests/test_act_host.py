"""The epilogue arithmetic behind every int8 kernel (fast-dnn_amd/csrc/fdnn_act.hpp: dequant, the reference's table index
lut_index and its half-step form lut2_index, pack4, the logit's exp), checked on the host alone: the stand-alone checker
tests/host/act_check.cpp holds the half-step form to lut_index -- as indices and, through build_sigmoid_lut and the loader's
lut2_build, as bytes -- over every float near a half-step boundary and a stride of all floats the loader admits; it is built
with the address and undefined-behaviour sanitizers (with fdnn_model.cpp, whose tables it reads) and run as a child process.
CPU only.  The kernels' use of it: tests/test_gpu_parity.py, tests/test_gpu_model_limits.py."""
import os
import subprocess

from conftest import ROOT


def test_act_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "act_check")
    src = os.path.join(ROOT, "tests", "host", "act_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, os.path.join(inc, "fdnn_model.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    print(run.stdout)
    assert "act ok" in run.stdout
