"""Dense scoring with a top-k return, the half that needs no GPU: the stand-alone checker of fdnn_topk.hpp and of the kTopk
arm of the scoring loop's batch plan under the sanitizers, the host restatement (api.topk_ref) against the contract stated in
numpy on the planted rows of tests/test_gpu_topk_rows.py, and that the new entry points are declared, exported and bound."""
import os
import re
import subprocess

import numpy as np
import pytest

import topk_cases as TC
from conftest import ROOT
from fast_dnn_amd import api

NAMES = ("fdnn_topk_rows_device", "fdnn_ctx_output_topk", "fdnn_ctx_output_topk_device", "fdnn_calculate_topk", "fdnn_calculate_topk_raw",
         "fdnn_calculate_topk_device", "fdnn_server_submit_topk", "fdnn_server_submit_raw_topk", "fdnn_debug_topk_launches",
         "fdnn_debug_set_topk_kernel", "fdnn_debug_topk_ref")


def test_topk_header_and_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "topk_check")
    src = os.path.join(ROOT, "tests", "host", "topk_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "topk ok" in run.stdout


def test_topk_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fdnn.h")).read()
    for name in NAMES:
        assert name in api.SIGNATURES and hasattr(api.lib(), name) and "FDNN_API int " + name + "(" in header, name
    for cls, methods in ((api.QuantizedDnn, ("calculateTopK", "calculateTopKRaw", "calculate_topk_device")),
                         (api.LazyContext, ("calculateOutputTopK", "calculateOutputTopKDevice")),
                         (api.ScoringServer, ("submitTopK", "submitRawTopK"))):
        for m in methods:
            assert callable(getattr(cls, m)), m
    for fn in ("topk_rows_device", "topk_ref", "topk_launches", "set_topk_kernel"):
        assert callable(getattr(api, fn)), fn
    assert len(api.topk_launches()) == 2
    with pytest.raises(api.FdnnError):
        api.set_topk_kernel(3)
    api.set_topk_kernel(0)


def test_no_recorder_name_starts_with_topk():
    assert not any(n.startswith("topk") for n in api.launch_names())  # counted apart from the recorder's table (fdnn_note.hpp)


def test_the_limits_are_the_headers():
    text = open(os.path.join(ROOT, "fast-dnn_amd", "csrc", "fdnn_topk.hpp")).read()
    max_k = int(re.search(r"constexpr int kTopkMaxK = (\d+);", text).group(1))
    resident = int(re.search(r"constexpr int kTopkResidentWidth = (\d+);", text).group(1))
    assert max_k == api.TOPK_MAX_K == 256 and resident == api.TOPK_RESIDENT_WIDTH >= 16384
    assert api.topk_limits() == (max_k, resident)


def test_the_key_in_numpy_is_the_contracts():
    v = np.array([0xffc00000, 0xff800000, 0xbf800000, 0x80000000, 0x00000000, 0x3f800000, 0x7f800000, 0x7fc00000], np.uint32).view(np.float32)
    k = TC.key(v[None, :])[0]
    assert k.dtype == np.uint32 and (np.diff(k.astype(np.int64)) > 0).all()
    assert k[3] == 0x7fffffff and k[4] == 0x80000000


@pytest.mark.parametrize("width", TC.WIDTHS)
def test_topk_ref_is_the_numpy_selection_on_the_planted_rows(width):
    n = 130 if width <= 1001 else 5  # (the literal lexsort on the widest rows: a few of them)
    for kind in TC.KINDS:
        rows = None
        for k in TC.ks_for(width):
            if rows is None or kind == "plateau":
                rows = TC.rows_of(kind, n, width, k)
                before = rows.view(np.uint32).copy()
            want_nodes, want_vals = TC.select_lexsort(rows, k)
            fast_nodes, fast_vals = TC.select(rows, k)
            assert np.array_equal(fast_nodes, want_nodes) and np.array_equal(fast_vals, want_vals), (kind, k)
            nodes, vals = api.topk_ref(rows, k)
            assert nodes.dtype == np.int32 and vals.dtype == np.float32
            assert np.array_equal(nodes, want_nodes), (kind, k)
            assert np.array_equal(vals.view(np.uint32), want_vals), (kind, k)
            assert np.array_equal(rows.view(np.uint32), before)
            if kind == "equal":
                assert (nodes == np.arange(k)[None, :]).all()
            if kind == "plateau":  # exactly k - 1 values above the plateau, and the lowest tie closes the result
                assert (rows > 0.5).sum(1).tolist() == [k - 1] * n and (vals[:, -1] == 0.5).all()
                assert nodes[:, -1].tolist() == [int(np.nonzero(rows[f] == 0.5)[0][0]) for f in range(n)]


def test_topk_ref_prefix_property():
    rows = TC.rows_of("alternating", 3, 300, 1)
    rows[1] = TC.rows_of("special", 1, 300, 1)[0]
    prev = None
    for k in range(1, 257):
        nodes, vals = api.topk_ref(rows, k)
        if prev is not None:
            assert np.array_equal(nodes[:, :-1], prev[0]) and np.array_equal(vals.view(np.uint32)[:, :-1], prev[1])
        prev = (nodes, vals.view(np.uint32).copy())


@pytest.mark.parametrize("width,k", [(10, 0), (10, 11), (1000, 257), (0, 1)])
def test_topk_ref_refuses_bad_arguments(width, k):
    with pytest.raises(api.FdnnError):
        api.topk_ref(np.zeros((2, width), np.float32), k)
