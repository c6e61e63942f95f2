"""Lazy output for a shared node set, the half that needs no GPU: the validator, the stand-alone checker of fdnn_set.hpp under
the sanitizers (the guard from a node to a weight-row offset, the tile plan), and -- from the oracle alone -- the premises of
tests/test_gpu_lazy_set.py: the finish kernel's normative sum order over the set's uniform rows, restated in numpy fp32
(lazy_lists_cases.emulate), is within 2e-6 of Oracle.lazy on every GPU fixture and within the relative bound on the ladder net."""
import os
import re
import subprocess

import numpy as np
import pytest

import lazy_lists_cases as LC
import lazy_set_cases as SC
import softmax_ref as SR
from conftest import ROOT
from fast_dnn_amd import api, formats as F

O = 1000


def test_validator_accepts_what_the_contract_allows():
    assert api.set_check([], O) == 0  # len == 0: every row reads 1 / O
    assert api.set_check([0], O) == 0 and api.set_check([O - 1], O) == 0 and api.set_check([0, O - 1], O) == 0
    assert api.set_check(np.arange(O), O) == 0  # len == O: the dense soft-max


@pytest.mark.parametrize("what,nodes", [
    ("unsorted", [3, 2, 7]),
    ("a duplicate", [1, 4, 4]),
    ("negative", [-1, 5]),
    ("== O", [5, O]),
    ("len > O", list(range(O + 1))),
])
def test_validator_rejects(what, nodes):
    assert api.set_check(nodes, O) == -1, what


def test_set_entry_points_are_declared_and_bound():
    names = ("fdnn_ctx_lazy_output_set", "fdnn_ctx_lazy_output_set_device", "fdnn_calculate_lazy_set", "fdnn_debug_set_check",
             "fdnn_debug_ctx_set_acc", "fdnn_debug_set_launches", "fdnn_debug_set_kernel")
    header = open(os.path.join(ROOT, "include", "fdnn.h")).read()
    for name in names:
        assert name in api.SIGNATURES and hasattr(api.lib(), name) and name + "(" in header
    assert len(api.set_launches()) == 3
    assert not any(n.startswith(("set.", "lists")) for n in api.launch_names())  # counted apart from the recorder's table (fdnn_note.hpp)
    with pytest.raises(api.FdnnError):
        api.set_kernel(3)
    api.set_kernel(0)


def test_the_tile_sizes_are_the_headers():
    text = open(os.path.join(ROOT, "fast-dnn_amd", "csrc", "fdnn_set.hpp")).read()
    assert int(re.search(r"constexpr int kNodeTile = (\d+);", text).group(1)) == api.SET_NODE_TILE == SC.NT
    assert int(re.search(r"constexpr int kFrameTile = (\d+);", text).group(1)) == api.SET_FRAME_TILE == SC.FT


def test_set_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "set_check")
    src = os.path.join(ROOT, "tests", "host", "set_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "set ok" in run.stdout


@pytest.fixture(scope="module")
def fixtures(mid_model_path, sat_model_path, tiny_model_path, net_model_path):
    yield {"mid": mid_model_path, "sat": sat_model_path, "tiny": tiny_model_path, "full": net_model_path}
    SC.release()


@pytest.mark.parametrize("name", list(SC.CASES))
def test_the_normative_order_meets_the_bars_on_uniform_rows(fixtures, name):
    """Exact exps summed in the finish kernel's order over the set's uniform rows: within 2e-6 of Oracle.lazy at the listed
    entries and at the inactive values; an empty set reads exactly 1 / O; the overflowing set has the oracle's NaN / 0
    pattern; the ladder cases stay within lazy_lists_cases.relative_bound of float64."""
    r = SC.reference(name, fixtures)
    n, L = r["x"].shape[0], r["nodes"].size
    probs, inactive = LC.emulate(r["z"], r["row_ptr"], r["list_nodes"], r["O"])
    probs = probs.reshape(n, L)
    assert np.array_equal(np.isnan(probs), np.isnan(r["want_probs"]))
    ok = ~np.isnan(probs)
    assert np.abs(probs[ok] - r["want_probs"][ok]).max(initial=0.0) <= SC.TIGHT
    rows = ~np.isnan(r["want_inactive"])
    assert np.abs(inactive[rows] - r["want_inactive"][rows]).max(initial=0.0) <= SC.TIGHT
    if L == 0:
        assert (inactive == np.float32(1.0) / np.float32(r["O"])).all()
    if name == "tail.ovf.hot":
        assert (np.isnan(r["want_probs"]).sum(1) == 4).all() and (r["want_inactive"] == 0).all()
        assert (r["want_probs"][~np.isnan(r["want_probs"])] == 0).all()
    if name == "tail.ovf.cold":
        assert np.isfinite(r["want_rows"]).all() and (r["want_inactive"] > 0).all()
    if name in SC.RELATIVE:
        p64 = SR.softmax64(r["z"])
        assert (p64 >= SR.TINY).all()  # no entry in softmax_ref's second class
        got = F.lists_to_rows(r["row_ptr"], r["list_nodes"], probs.ravel(), inactive, r["O"])
        for f in range(n):
            listed = r["masks"][f] != 0
            rel = np.abs(got[f].astype(np.float64) / p64[f] - 1.0)
            assert (rel <= LC.relative_bound(r["z"][f], listed, p64[f])).all(), (name, f)


def test_the_cases_cover_what_they_are_there_for():
    lens = {SC.CASES[f"mid.len{L}"].build().size for L in (0, 1, SC.NT - 1, SC.NT, SC.NT + 1, 2 * SC.NT + 1, 1000)}
    assert lens == {0, 1, SC.NT - 1, SC.NT, SC.NT + 1, 2 * SC.NT + 1, 1000}
    for L in (SC.NT - 1, SC.NT, SC.NT + 1, 2 * SC.NT + 1, 1000):
        nd = SC.CASES[f"mid.len{L}"].build()
        assert nd[0] == 0 and nd[-1] == 999
        assert {c for _, c in SC.CASES[f"mid.len{L}"].ranges} == {1, SC.FT - 1, SC.FT + 1, 100}
    assert SC.CASES["odd.lad251"].build()[-1] == 250
    assert SC.CASES["mid.first7"].ranges[0][0] == 7 and SC.CASES["mid.first7"].n == 100
