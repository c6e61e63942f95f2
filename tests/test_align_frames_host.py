"""The frames form of the best path over alignment graphs, the half that needs no GPU: the stand-alone checker of
fdnn_align_frames.hpp under the sanitizers (tests/host/align_frames_check.cpp)."""
import os
import subprocess

from conftest import ROOT


def test_align_frames_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "align_frames_check")
    clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    cc = subprocess.run([clang if os.path.exists(clang) else "g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "fast-dnn_amd", "csrc"),
                         os.path.join(ROOT, "tests", "host", "align_frames_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0 and "align frames ok" in run.stdout, run.stdout + run.stderr  # (the first failure ends it)
