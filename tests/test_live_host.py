"""Live utterances through the scoring loop, the part that needs no GPU: the position arithmetic that fdnn_stream_push and the
loop's live handles share (fast-dnn_amd/csrc/fdnn_stream_plan.hpp) and the batches plan_batch makes of live pushes
(fdnn_server_plan.hpp), stated by the stand-alone checker tests/host/stream_plan_check.cpp, which is built with the address
and undefined-behaviour sanitizers and run as a child process; and the new entry points' presence in the library, the
header and the Python binding.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from fast_dnn_amd import api

LIVE = ("fdnn_server_live_open", "fdnn_server_live_close", "fdnn_server_live_reset", "fdnn_server_live_position", "fdnn_server_live_push",
        "fdnn_server_live_push_topk", "fdnn_server_live_push_pool", "fdnn_server_live_push_set", "fdnn_debug_splice_table",
        "fdnn_debug_live_launches", "fdnn_debug_server_hold")


def test_stream_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "stream_plan_check")
    src = os.path.join(ROOT, "tests", "host", "stream_plan_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "stream plan ok" in run.stdout


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fdnn.h")).read()
    L = api.lib()
    for name in LIVE:
        assert name + "(" in header and name in api.SIGNATURES and hasattr(L, name), name
    for method in ("push", "pushTopK", "pushPool", "pushSet", "reset", "position", "close"):
        assert callable(getattr(api.LiveStream, method))
    assert callable(api.ScoringServer.openLive) and callable(api.ScoringServer.hold) and callable(api.splice_table)


def test_the_table_kernel_is_not_a_recorded_launch_name():
    """The table kernel is counted behind its own entry (live_launches), as the list, set, top-k and pool kernels are: the
    launch recorder's table keeps its names, every one of which has a ledger case."""
    assert not any("table" in name or "live" in name for name in api.launch_names())
    counts = api.live_launches()  # (process-wide: zero here only when no GPU test ran before in this process)
    assert set(counts) == {"launches", "max_segs"} and (counts["launches"] == 0) == (counts["max_segs"] == 0)


def test_splice_table_refuses_malformed_tables_without_a_device():
    raw = np.zeros((4, 39), dtype=np.float32)
    ok = [[0, 0, 0, 3]]
    for segs, rows, width in (([[1, 0, 0, 3]], 4, 432),            # the first segment does not start at row 0
                              ([[0, 0, 0, 3], [0, 1, 0, 3]], 4, 432),  # rows do not ascend
                              ([[0, 0, 0, 3], [4, 1, 0, 3]], 4, 432),  # a segment beyond the rows
                              ([[0, 0, 3, 2]], 4, 432),            # lo > hi
                              ([[0, 0, 4, 9]], 4, 432),            # no frame of the buffer
                              (ok, 4, 430), (ok, 4, 428), (ok, 0, 432)):  # width not a multiple of 4 / too narrow; no rows
        with pytest.raises(api.FdnnError) as e:
            api.splice_table(list(range(-5, 6)), 39, width, raw, segs, rows, True)
        assert e.value.code == api.FDNN_E_ARG
