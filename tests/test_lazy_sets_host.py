"""Lazy output for per-segment node sets, the half that needs no GPU: the validator through the C-ABI, every new symbol
declared, exported and bound, the launch counters, formats.sets_to_lists against fdnn_sets.hpp's row pointer, and the
stand-alone checker of fdnn_sets.hpp and of the scoring loop's plan for set submissions under the sanitizers
(tests/host/sets_check.cpp).  That the normative sum order meets the bars of tests/test_gpu_lazy_sets.py on the (row, set)
pairs it scores is tests/test_lazy_set_host.py's result: every segment there is rows of a lazy_set_cases case with that
case's set."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from fast_dnn_amd import api, formats as F

O = 1000
NAMES = ("fdnn_ctx_lazy_output_sets", "fdnn_ctx_lazy_output_sets_device", "fdnn_calculate_lazy_sets", "fdnn_debug_sets_check",
         "fdnn_debug_ctx_sets_acc", "fdnn_debug_sets_launches", "fdnn_server_submit_lazy_set", "fdnn_server_submit_raw_set")


def test_validator_accepts_what_the_contract_allows():
    # an empty segment, a zero-length set, node 0 and node O - 1, rows up to the context's last, a first row above 0
    assert api.sets_check([0, 1, 32, 32, 65, 100], [0, 2, 2, 3, 5, 6], [0, O - 1, 7, 1, 2, O - 1], O, 100) == 0
    assert api.sets_check([5, 5], [0, 0], [], O, 100) == 0
    assert api.sets_check([7], [0], [], O, 100) == 0  # no segment: a no-op
    assert api.sets_check([0, 10, 20], [0, 2, 4], [5, 9, 1, 2], O, 100) == 0  # ascending inside a set, not across sets
    assert api.sets_check([0, 100], [0, O], np.arange(O), O, 100) == 0  # len == O: the dense soft-max


@pytest.mark.parametrize("what,seg_rows,set_ptr,nodes,want", [
    ("seg_rows[0] < 0", [-1, 3], [0, 1], [4], -1),
    ("set_ptr[0] != 0", [0, 3, 6], [1, 2, 3], [4, 5, 6], -1),
    ("rows run backwards", [0, 10, 5], [0, 1, 2], [4, 5], -2),
    ("rows past the context", [0, 10, 101], [0, 1, 2], [4, 5], -2),
    ("a set's range runs backwards", [0, 10, 20, 30], [0, 2, 1, 3], [4, 5, 6], -2),
    ("unsorted", [0, 10, 20], [0, 2, 5], [1, 2, 3, 2, 7], -2),
    ("a duplicate", [0, 10, 20], [0, 2, 5], [1, 2, 4, 4, 7], -2),
    ("negative", [0, 10, 20], [0, 2, 4], [-1, 5, 1, 2], -1),
    ("== O", [0, 10, 20, 30], [0, 1, 2, 4], [1, 2, 5, O], -3),
    ("len > O", [0, 10], [0, O + 1], list(range(O + 1)), -1),
    ("set_ptr past the nodes", [0, 10, 20], [0, 1, 5], [1, 2], -2),
])
def test_validator_names_the_first_malformed_segment(what, seg_rows, set_ptr, nodes, want):
    assert api.sets_check(seg_rows, set_ptr, nodes, O, 100) == want, what


def test_sets_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fdnn.h")).read()
    for name in NAMES:
        assert name in api.SIGNATURES and hasattr(api.lib(), name) and name + "(" in header, name
    assert len(api.sets_launches()) == 3 and len(api.set_launches()) == 3
    assert not any(n.startswith(("set.", "sets.", "lists")) for n in api.launch_names())  # counted apart from the recorder's table
    for name in ("calculateForOutputNodeSets", "calculateForOutputNodeSetsDevice", "setsAccumulators"):
        assert hasattr(api.LazyContext, name)
    assert hasattr(api.QuantizedDnn, "calculateLazySets")
    assert hasattr(api.ScoringServer, "submitLazySet") and hasattr(api.ScoringServer, "submitRawSet")


def test_sets_to_lists_is_the_list_contract_of_the_same_call():
    seg_rows, set_ptr = [3, 4, 35, 35, 68, 103], [0, 3, 3, 4, 6, 8]
    nodes = np.array([5, 6, 9, 1, 0, 999, 2, 3], np.int32)
    row_ptr, list_nodes = F.sets_to_lists(seg_rows, set_ptr, nodes)
    assert row_ptr.dtype == np.int32 and list_nodes.dtype == np.int32 and row_ptr.size == 101 and row_ptr[0] == 0
    assert api.lists_check(row_ptr, list_nodes, O) == 0
    want = []
    for s in range(5):
        want += [nodes[set_ptr[s]:set_ptr[s + 1]]] * (seg_rows[s + 1] - seg_rows[s])
    for r in range(100):
        assert np.array_equal(list_nodes[row_ptr[r]:row_ptr[r + 1]], want[r]), r
    # segment s's block starts at the sum of rows x len before it
    assert row_ptr[1] == 3 and row_ptr[32] == 3 and row_ptr[65] == 3 + 33 * 2 and row_ptr[100] == 3 + 33 * 2 + 35 * 2
    rp, nd = F.sets_to_lists([0], [0], [])
    assert rp.tolist() == [0] and nd.size == 0


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sets") / "sets_check")
    src = os.path.join(ROOT, "tests", "host", "sets_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    return exe


def test_sets_header_and_server_plan_under_sanitizers(checker):
    run = subprocess.run([checker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "sets ok" in run.stdout


@pytest.mark.parametrize("seg_rows,set_ptr", [
    ([0, 1, 32, 32, 65, 100], [0, 65, 65, 66, 195, 259]),
    ([7, 7, 8], [0, 4, 4]),
    ([0, 130], [0, 1]),
])
def test_the_headers_row_pointer_is_sets_to_lists(checker, seg_rows, set_ptr):
    run = subprocess.run([checker, "rowptr"] + [str(v) for v in seg_rows] + ["/"] + [str(v) for v in set_ptr], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    row_ptr, _ = F.sets_to_lists(seg_rows, set_ptr, np.arange(set_ptr[-1], dtype=np.int32))
    assert [int(v) for v in run.stdout.split()] == row_ptr.tolist()
