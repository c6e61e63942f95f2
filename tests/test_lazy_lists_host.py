"""Lazy output by active-node lists, the half that needs no GPU: the validator, the list <-> mask helpers, the stand-alone
checker of fdnn_lists.hpp under the sanitizers, and -- from the oracle alone -- the premises of tests/test_gpu_lazy_lists.py:
the finish kernel's normative sum order, restated in numpy fp32, is within 2e-6 of Oracle.lazy on every GPU fixture, and the
ladder net's masked logits keep every float64 probability a normal fp32 (no entry in softmax_ref's second class)."""
import os
import subprocess

import numpy as np
import pytest

import lazy_lists_cases as LC
import softmax_ref as SR
from conftest import ROOT
from fast_dnn_amd import api, formats as F

O = 1000


def _lists(rows):
    row_ptr = np.zeros(len(rows) + 1, np.int32)
    row_ptr[1:] = np.cumsum([len(r) for r in rows])
    return row_ptr, np.array([v for r in rows for v in r], np.int32)


def test_validator_accepts_what_the_contract_allows():
    assert api.lists_check(*_lists([[], list(range(O)), [0], [O - 1], []]), O) == 0
    assert api.lists_check(*_lists([[]]), O) == 0
    assert api.lists_check(*_lists([[0, O - 1]]), O) == 0
    assert api.lists_check(*F.masks_to_lists(F.generate_masks(50, O, 0.4, 0.03, seed=2)), O) == 0


@pytest.mark.parametrize("what,rows,row", [
    ("a descending pair", [[1, 2], [5, 4], [7]], 1),
    ("a duplicate", [[1, 2], [3], [7, 7]], 2),
    ("-1", [[-1]], 0),
    ("-1 later", [[0], [], [2, 3], [-1, 5]], 3),
    ("O", [[0], [5, O]], 1),
])
def test_validator_rejects_and_names_the_row(what, rows, row):
    assert api.lists_check(*_lists(rows), O) == -(row + 1), what


def test_validator_rejects_a_bad_row_ptr():
    rp, nd = _lists([[1], [2, 3], [4]])
    shifted = rp.copy()
    shifted[0] = 1
    assert api.lists_check(shifted, nd, O) == -1  # row_ptr[0] != 0 answers as row 0
    dec = rp.copy()
    dec[2] = 0  # row 1 runs backwards
    assert api.lists_check(dec, nd, O) == -2
    long = rp.copy()
    long[3] = 9  # past the node array: never read
    assert api.lists_check(long, nd, O) == -3


def test_masks_to_lists_and_back():
    m = F.generate_masks(40, 251, 0.4, 0.03, seed=4)
    m[0] = 0
    m[1] = 1
    m[2] = 0
    m[2, 250] = 1
    rp, nd = F.masks_to_lists(m)
    assert rp.dtype == np.int32 and nd.dtype == np.int32 and rp[0] == 0 and rp[-1] == nd.size == int((m != 0).sum())
    assert api.lists_check(rp, nd, 251) == 0
    probs = np.arange(1, nd.size + 1, dtype=np.float32)
    inactive = -np.arange(1, 41, dtype=np.float32)
    rows = F.lists_to_rows(rp, nd, probs, inactive, 251)
    assert rows.shape == (40, 251) and np.array_equal(rows > 0, m != 0)
    assert np.array_equal(rows[m != 0], probs)  # row-major: the entries' own order
    assert all((rows[f][m[f] == 0] == inactive[f]).all() for f in range(40))
    assert np.array_equal(np.concatenate(F.masks_to_lists(rows > 0)), np.concatenate((rp, nd)))


def test_list_entry_points_are_declared_and_bound():
    names = ("fdnn_ctx_lazy_output_lists", "fdnn_ctx_lazy_output_lists_device", "fdnn_calculate_lazy_lists", "fdnn_debug_lists_check",
             "fdnn_debug_ctx_lists_acc", "fdnn_debug_lists_launches")
    header = open(os.path.join(ROOT, "include", "fdnn.h")).read()
    for name in names:
        assert name in api.SIGNATURES and hasattr(api.lib(), name) and name + "(" in header
    assert len(api.lists_launches()) == 3
    assert not any(n.startswith("lists") for n in api.launch_names())  # counted apart from the recorder's table (fdnn_note.hpp)


def test_lists_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lists_check")
    src = os.path.join(ROOT, "tests", "host", "lists_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "lists ok" in run.stdout


@pytest.fixture(scope="module")
def fixtures(mid_model_path, sat_model_path, tiny_model_path, net_model_path):
    yield {"mid": mid_model_path, "sat": sat_model_path, "tiny": tiny_model_path, "full": net_model_path}
    LC.release()


@pytest.mark.parametrize("name", list(LC.CASES))
def test_the_normative_order_meets_the_absolute_bar(fixtures, name):
    """Premise of the GPU bounds, from the oracle alone: exact exps summed in the finish kernel's order are within 2e-6 of
    Oracle.lazy at the listed entries and at the inactive values; an overflowing row has the oracle's NaN / 0 pattern."""
    r = LC.reference(name, fixtures)
    probs, inactive = LC.emulate(r["z"], r["row_ptr"], r["nodes"], r["O"])
    assert np.array_equal(np.isnan(probs), np.isnan(r["want_probs"]))
    ok = ~np.isnan(probs)
    assert np.abs(probs[ok] - r["want_probs"][ok]).max(initial=0.0) <= LC.TIGHT
    rows = ~np.isnan(r["want_inactive"])
    assert np.abs(inactive[rows] - r["want_inactive"][rows]).max(initial=0.0) <= LC.TIGHT
    lens = np.diff(r["row_ptr"])
    assert (inactive[lens == 0] == np.float32(1.0) / np.float32(r["O"])).all()  # an empty row: 1 / O
    if name == "tail.ovf.n33":
        hot = np.isnan(r["want_probs"])
        assert hot.sum() == 4 * 17 and (r["want_probs"][~hot & np.isin(r["rows"], np.arange(0, 33, 2))] == 0).all()
        assert (r["want_inactive"][::2] == 0).all() and (r["want_inactive"][1::2] > 0).all()
    if name == "full.n64":
        assert lens.max() == 8000 and (lens == 8).sum() >= 30 and (lens == 80).sum() >= 30
    if name == "odd.lad251.n33":
        assert (r["nodes"] == 250).sum() >= 29


@pytest.mark.parametrize("name", LC.RELATIVE)
def test_ladder_fixtures_have_no_second_class_entries(fixtures, name):
    """softmax64 of the masked logits is >= 2^-126 everywhere, so the second-class share of the GPU test is 0 by construction;
    and the relative bound, evaluated on the exact restatement, holds with room (it has no exp error: c_e's share is slack)."""
    r = LC.reference(name, fixtures)
    p64 = SR.softmax64(r["z"])
    assert (p64 >= SR.TINY).all()
    probs, inactive = LC.emulate(r["z"], r["row_ptr"], r["nodes"], r["O"])
    got = F.lists_to_rows(r["row_ptr"], r["nodes"], probs, inactive, r["O"])
    for f in range(got.shape[0]):
        listed = r["masks"][f] != 0
        b = LC.relative_bound(r["z"][f], listed, p64[f])
        rel = np.abs(got[f].astype(np.float64) / p64[f] - 1.0)
        assert (rel <= b).all(), (name, f, float((rel / b).max()))
