"""Lazy output by lists over per-frame-group node unions (fdnn_model_set_lists_union; fdnn_lists_union.hip), the half that
needs no GPU: the stand-alone checker of fdnn_lists_union.hpp under the sanitizers, the host restatement through the C ABI
against a numpy union, and the declarations.  The GPU half: tests/test_gpu_lazy_lists_union.py."""
import os
import subprocess

import numpy as np
import pytest

import lazy_lists_cases as LC
from conftest import ROOT
from fast_dnn_amd import api, formats as F


def test_lists_union_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lists_union_check")
    src = os.path.join(ROOT, "tests", "host", "lists_union_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "lists union ok" in run.stdout


def numpy_union(row_ptr, nodes, group_tiles):
    """-> (u_len, u_nodes, pos) as fdnn.h lays them out, from np.unique per group of 32 * group_tiles rows."""
    n, rows = row_ptr.size - 1, 32 * group_tiles
    u_len = np.zeros(-(-n // rows), np.int32)
    u_nodes = np.full(nodes.size, -1, np.int32)
    pos = np.full(nodes.size, -1, np.int32)
    for q in range(u_len.size):
        b, e = int(row_ptr[q * rows]), int(row_ptr[min(n, (q + 1) * rows)])
        u, inv = np.unique(nodes[b:e], return_inverse=True)
        u_len[q] = u.size
        u_nodes[b:b + u.size] = u
        pos[b:e] = inv
    return u_len, u_nodes, pos


def _special_masks():
    """65 rows of 251 nodes: slowly changing 5 % sets, rows 32 .. 63 empty (a group without entries for g = 1), row 64 full."""
    m = F.generate_masks(65, 251, 0.05, 0.03, seed=65)
    m[32:64] = 0
    m[64] = 1
    return m


@pytest.mark.parametrize("case", ["mid.n100.s5", "special"])
@pytest.mark.parametrize("group_tiles", [1, 2, 8])
def test_union_ref_through_the_c_abi_equals_a_numpy_union(case, group_tiles):
    masks = _special_masks() if case == "special" else np.ascontiguousarray(LC.CASES[case][2](), dtype=np.int8)
    row_ptr, nodes = F.masks_to_lists(masks)
    u_len, u_nodes, pos = api.lists_union_ref(row_ptr, nodes, masks.shape[1], group_tiles)
    want = numpy_union(row_ptr, nodes, group_tiles)
    assert np.array_equal(u_len, want[0]) and np.array_equal(u_nodes, want[1]) and np.array_equal(pos, want[2])
    # what the layout promises: a union is no longer than its group's entry range, and the chunks fit the score grid
    rows = 32 * group_tiles
    ends = row_ptr[np.minimum(np.arange(1, u_len.size + 1) * rows, row_ptr.size - 1)]
    assert (u_len <= ends - row_ptr[::rows][:u_len.size]).all()
    assert int((-(-u_len // 64)).sum()) <= nodes.size // 64 + u_len.size
    if case == "special" and group_tiles == 1:
        assert u_len[1] == 0 and u_len[2] == 251
    # generate_masks' churn is a share of the LAYER per frame: a union grows by at most int(O * churn) nodes per row
    if case == "mid.n100.s5":
        first_rows = np.diff(row_ptr)[::rows][:u_len.size]
        assert (u_len[1:] <= first_rows[1:] + (rows - 1) * int(1000 * 0.03)).all()  # (group 0 holds the planted full row)


def test_union_ref_rejects_what_the_validator_rejects():
    rp, nd = np.array([0, 2], np.int32), np.array([5, 5], np.int32)
    with pytest.raises(api.FdnnError) as e:
        api.lists_union_ref(rp, nd, 100, 1)
    assert e.value.code == api.FDNN_E_ARG
    with pytest.raises(api.FdnnError):
        api.lists_union_ref(np.array([0, 1], np.int32), np.array([3], np.int32), 100, 9)  # group_tiles is 1 .. 8


def test_union_entry_points_are_declared_and_bound():
    names = ("fdnn_model_set_lists_union", "fdnn_debug_lists_union_launches", "fdnn_debug_ctx_lists_union", "fdnn_debug_lists_union_ref")
    header = open(os.path.join(ROOT, "include", "fdnn.h")).read()
    for name in names:
        assert name in api.SIGNATURES and hasattr(api.lib(), name) and name + "(" in header
    assert "dnn.cc:355-392" in header[header.index("fdnn_debug_lists_union_launches") - 1200:header.index("fdnn_debug_lists_union_launches")]
    assert len(api.lists_union_launches()) == 4
    assert not any("union" in n for n in api.launch_names())  # counted apart from the recorder's table (fdnn_note.hpp)
    assert hasattr(api.QuantizedDnn, "setListsUnion")


def test_the_tile_header_and_the_binding_agree():
    """api._union_buffers sizes u_len by the set kernel's frame tile; fdnn_lists_union.hpp's groups are made of the same tiles."""
    text = open(os.path.join(ROOT, "fast-dnn_amd", "csrc", "fdnn_lists_union.hpp")).read()
    assert "set::kFrameTile * group_tiles" in text and api.SET_FRAME_TILE == 32
