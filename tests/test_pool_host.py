"""Class posteriors (the dense soft-max pooled over a node -> class map), the half that needs no GPU: the stand-alone checker of
fdnn_pool.hpp and of the kPool arm of the scoring loop's batch plan under the sanitizers, the host restatement (api.pool_ref)
against the contract stated in numpy (tests/pool_cases.py) and against float64 within the derived bound, the condition that
keeps the byte comparison from being blind, and that the new entry points are declared, exported and bound."""
import os
import re
import subprocess

import numpy as np
import pytest

import pool_cases as PC
import topk_cases as TC
from conftest import ROOT
from fast_dnn_amd import api

NAMES = ("fdnn_pool_rows_device", "fdnn_ctx_output_pool", "fdnn_ctx_output_pool_device", "fdnn_calculate_pool", "fdnn_calculate_pool_raw",
         "fdnn_calculate_pool_device", "fdnn_server_submit_pool", "fdnn_server_submit_raw_pool", "fdnn_debug_pool_launches",
         "fdnn_debug_set_pool_kernel", "fdnn_debug_pool_ref", "fdnn_debug_pool_limits", "fdnn_pool_width", "fdnn_pool_classes")


def test_pool_header_and_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pool_check")
    src = os.path.join(ROOT, "tests", "host", "pool_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "pool ok" in run.stdout


def test_pool_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fdnn.h")).read()
    for name in NAMES:
        assert name in api.SIGNATURES and hasattr(api.lib(), name) and "FDNN_API int " + name + "(" in header, name
    for name, decl in (("fdnn_pool_create", "FDNN_API fdnn_pool *fdnn_pool_create("), ("fdnn_pool_free", "FDNN_API void fdnn_pool_free(")):
        assert name in api.SIGNATURES and hasattr(api.lib(), name) and decl in header, name
    at = header.index("fdnn_pool_create")
    assert "dnn.cc:428-454" in header[at - 4000:at + 4000]  # cited as an extension of CalculateOutput
    for cls, methods in ((api.QuantizedDnn, ("calculatePool", "calculate_pool", "calculatePoolRaw", "calculate_pool_device")),
                         (api.LazyContext, ("calculateOutputPool", "calculateOutputPoolDevice")),
                         (api.ScoringServer, ("submitPool", "submitRawPool")), (api.ClassPool, ("width", "classes", "rows_device", "delete"))):
        for m in methods:
            assert callable(getattr(cls, m)), m
    for fn in ("pool_ref", "pool_launches", "set_pool_kernel", "pool_limits"):
        assert callable(getattr(api, fn)), fn
    assert len(api.pool_launches()) == 2
    with pytest.raises(api.FdnnError):
        api.set_pool_kernel(3)
    api.set_pool_kernel(0)


def test_no_recorder_name_starts_with_pool():
    assert not any(n.startswith("pool") for n in api.launch_names())  # counted apart from the recorder's table (fdnn_note.hpp)


def test_the_limits_are_the_headers():
    text = open(os.path.join(ROOT, "fast-dnn_amd", "csrc", "fdnn_pool.hpp")).read()
    lanes = int(re.search(r"constexpr int kPoolLanes = (\d+);", text).group(1))
    resident = int(re.search(r"constexpr int kPoolResidentWidth = (\d+);", text).group(1))
    assert lanes == api.POOL_LANES and resident == api.POOL_RESIDENT_WIDTH
    assert api.pool_limits() == (lanes, resident)
    assert lanes & (lanes - 1) == 0 and 4 * (resident + 4) <= 160 * 1024


def test_the_kernel_file_is_built_without_flush_to_zero_or_fast_math():
    mk = open(os.path.join(ROOT, "fast-dnn_amd", "csrc", "Makefile")).read()
    for flag in ("-ffast-math", "-fgpu-flush-denormals-to-zero", "-funsafe-math-optimizations", "-fdenormal-fp-math", "-Ofast", "-fassociative-math"):
        assert flag not in mk, flag


@pytest.mark.parametrize("width", [1, 2, 17, 65, 251, 1001])
def test_vectorised_numpy_rule_is_the_literal_one(width):
    """tests/pool_cases.py states the rule twice; the scalar transcription holds the vectorised one on every map kind."""
    for kind in ("softmax", "special"):
        rows = TC.rows_of(kind, 3, width, 1)
        for mk in PC.MAP_KINDS:
            co, C = PC.map_of(mk, width)
            got = PC.pool_numpy(rows, co, C)
            mem = PC.members(co, C)
            if width > 300 and mk == "identity":
                mem_idx = range(0, C, 97)
            else:
                mem_idx = range(C)
            want = np.array([[PC.pool_literal(rows[r], mem[c]) for c in mem_idx] for r in range(rows.shape[0])], np.float32)
            assert PC.same_bytes(got[:, list(mem_idx)], want), (kind, mk)


@pytest.mark.parametrize("width", [1, 2, 63, 64, 65, 251, 1001, 8000])
def test_pool_ref_is_the_numpy_rule(width):
    n = 9 if width <= 1001 else 3
    for kind in TC.KINDS:
        rows = TC.rows_of(kind, n, width, 1)
        before = rows.view(np.uint32).copy()
        for mk in PC.MAP_KINDS:
            co, C = PC.map_of(mk, width)
            got = api.pool_ref(rows, co, C)
            assert got.dtype == np.float32 and got.shape == (n, C)
            assert PC.same_bytes(got, PC.pool_numpy(rows, co, C)), (kind, mk)
            if mk == "identity" and kind != "special":  # singletons: the value's own bits (no -0 in these rows)
                assert np.array_equal(got.view(np.uint32), before)
            if mk == "none":
                assert (got.view(np.uint32) == 0).all()  # empty classes: +0
        assert np.array_equal(rows.view(np.uint32), before)


def test_singletons_keep_their_bits_and_minus_zero_becomes_plus_zero():
    row = TC.SPECIALS[None, :].copy()
    got = api.pool_ref(row, np.arange(row.shape[1], dtype=np.int32), row.shape[1]).view(np.uint32)[0]
    want = row.view(np.uint32)[0].copy()
    nan = np.isnan(row[0])
    want[want == 0x80000000] = 0
    assert np.array_equal(got[~nan], want[~nan]) and np.isnan(got.view(np.float32)[nan]).all()


def test_every_listed_class_size_is_there():
    co, C = PC.map_of("sizes", 8000)
    assert C == len(PC.SIZES) and [int((co == c).sum()) for c in range(C)] == list(PC.SIZES)
    co, C = PC.map_of("gaps", 251)
    assert [int((co == c).sum()) > 0 for c in range(C)] == [True, False, True, False, True, False, True]


@pytest.mark.parametrize("width,C,mk", [(8000, 48, "interleaved"), (65, 2, "blocks2"), (8000, 11, "sizes"), (1001, 5, "blocks")])
def test_pool_ref_against_float64_within_the_derived_bound(width, C, mk):
    """|q_c - sum| <= d u / (1 - d u) * sum |p_i|, d = ceil(L / lanes) + 4: the restatement against something independent."""
    rows = TC.rows_of("softmax", 5, width, 1)
    if mk == "blocks2":
        co = (np.arange(width) * 2 // width).astype(np.int32)
    else:
        co, C = PC.map_of(mk, width)
    got = api.pool_ref(rows, co, C).astype(np.float64)
    worst = 0.0
    for c, m in enumerate(PC.members(co, C)):
        exact = rows[:, m].astype(np.float64).sum(1)
        mag = np.abs(rows[:, m].astype(np.float64)).sum(1)
        d = PC.depth(m.size)
        bound = d * PC.U / (1 - d * PC.U) * mag
        err = np.abs(got[:, c] - exact)
        assert (err <= bound + mag * 2.0 ** -40).all(), (c, m.size, float(err.max()), float(bound.min()))  # (2^-40: the float64 sum's own error)
        if m.size:
            worst = max(worst, float((err / np.maximum(PC.U * exact, 1e-300)).max()))
    print(f"W = {width}, C = {C}: largest error {worst:.2f} u q")


@pytest.mark.parametrize("width,C", [(8000, 48), (65, 2)])
def test_the_byte_comparison_is_not_blind(width, C):
    """On the soft-max fixture rows the rule's result differs from the sequential fp32 sum and from the float64 sum rounded
    to fp32 in at least one entry: a kernel that added in either of those orders would be caught by the byte comparison."""
    rows = TC.rows_of("softmax", 5, width, 1)
    co = (np.arange(width) % C).astype(np.int32)
    got = api.pool_ref(rows, co, C).view(np.uint32)
    seq = np.zeros((5, C), np.float32)
    f64 = np.zeros((5, C), np.float32)
    for c, m in enumerate(PC.members(co, C)):
        s = np.zeros(5, np.float32)
        for i in m:
            s = s + rows[:, i]
        seq[:, c] = s
        f64[:, c] = rows[:, m].astype(np.float64).sum(1).astype(np.float32)
    d_seq, d_f64 = int((got != seq.view(np.uint32)).sum()), int((got != f64.view(np.uint32)).sum())
    print(f"W = {width}, C = {C}: {d_seq} of {5 * C} entries differ from the sequential sum, {d_f64} from the rounded float64 sum")
    assert d_seq >= 1 and d_f64 >= 1


@pytest.mark.parametrize("co,C", [([0, 1, -2], 2), ([0, 2, 1], 2), ([0, 0, 0], 4), ([0, 0, 0], 0), ([0, 0, 0], -1)])
def test_pool_ref_refuses_bad_maps(co, C):
    with pytest.raises(api.FdnnError) as e:
        api.pool_ref(np.zeros((2, 3), np.float32), np.array(co, np.int32), C)
    assert e.value.code == api.FDNN_E_ARG


def test_an_all_minus_one_map_is_valid():
    out = api.pool_ref(np.ones((2, 3), np.float32), np.full(3, -1, np.int32), 2)
    assert out.shape == (2, 2) and (out.view(np.uint32) == 0).all()
