"""Decoder scores (the dense soft-max as ln p - log prior, fp32 or fp16), the half that needs no GPU: the stand-alone checker of
fdnn_loglik.hpp and of the loglik arm of the scoring loop's batch plan under the sanitizers, the host restatement
(api.loglik_ref) against the contract stated in numpy on api.ln_ref (tests/loglik_cases.py), the condition that keeps the byte
comparison from being blind, the checks on the handle's arguments, and that the new entry points are declared, exported and
bound."""
import os
import re
import subprocess

import numpy as np
import pytest

import loglik_cases as LC
import topk_cases as TC
from conftest import ROOT
from fast_dnn_amd import api

INT_NAMES = ("fdnn_loglik_width", "fdnn_loglik_type", "fdnn_loglik_rows_device", "fdnn_loglik_entries_device", "fdnn_ctx_output_loglik",
             "fdnn_ctx_output_loglik_device", "fdnn_calculate_loglik", "fdnn_calculate_loglik_raw", "fdnn_calculate_loglik_device",
             "fdnn_server_submit_loglik", "fdnn_server_submit_raw_loglik", "fdnn_server_live_push_loglik", "fdnn_debug_loglik_launches",
             "fdnn_debug_set_loglik_kernel", "fdnn_debug_loglik_ref", "fdnn_debug_loglik_entries_ref", "fdnn_debug_ln_ref")


def host_compiler():
    """The checker compares the fp16 conversion with _Float16, which the ROCm toolchain's clang++ has on every host it runs
    on (g++ only from version 12 on): the compiler beside hipcc, else g++."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    clang = os.path.join(rocm, "llvm", "bin", "clang++")
    return clang if os.path.exists(clang) else "g++"


def test_loglik_header_and_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "loglik_check")
    src = os.path.join(ROOT, "tests", "host", "loglik_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "loglik ok" in run.stdout
    assert "half conversion against _Float16" in run.stdout  # (the host compiler had the type: the comparison ran)


def test_loglik_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fdnn.h")).read()
    for name in INT_NAMES:
        assert name in api.SIGNATURES and hasattr(api.lib(), name) and "FDNN_API int " + name + "(" in header, name
    for name, decl in (("fdnn_loglik_create", "FDNN_API fdnn_loglik *fdnn_loglik_create("), ("fdnn_loglik_free", "FDNN_API void fdnn_loglik_free(")):
        assert name in api.SIGNATURES and hasattr(api.lib(), name) and decl in header, name
    at = header.index("fdnn_loglik_create")
    assert "dnn.cc:428-454" in header[at - 4000:at + 4000]  # cited as an extension of CalculateOutput
    assert "#define FDNN_LOGLIK_F32 0" in header and "#define FDNN_LOGLIK_F16 1" in header
    assert (api.LOGLIK_F32, api.LOGLIK_F16) == (0, 1)
    for cls, methods in ((api.QuantizedDnn, ("calculateLoglik", "calculate_loglik", "calculateLoglikRaw", "calculate_loglik_device")),
                         (api.LazyContext, ("calculateOutputLoglik", "calculateOutputLoglikDevice")),
                         (api.ScoringServer, ("submitLoglik", "submitRawLoglik")), (api.LiveStream, ("pushLoglik",)),
                         (api.Loglik, ("width", "type", "rows_device", "entries_device", "delete"))):
        for m in methods:
            assert callable(getattr(cls, m)), m
    for fn in ("loglik_ref", "loglik_entries_ref", "ln_ref", "loglik_launches", "set_loglik_kernel"):
        assert callable(getattr(api, fn)), fn
    assert len(api.loglik_launches()) == 3
    with pytest.raises(api.FdnnError):
        api.set_loglik_kernel(3)
    api.set_loglik_kernel(0)


def test_no_recorder_name_starts_with_loglik():
    assert not any(n.startswith("loglik") for n in api.launch_names())  # counted apart from the recorder's table (fdnn_note.hpp)


def test_the_bound_is_the_recorded_sweeps():
    """kLnMaxUlp is the exhaustive run's worst error rounded UP to the next 0.05 ulp, and that run covered every input."""
    text = open(os.path.join(ROOT, "fast-dnn_amd", "csrc", "fdnn_loglik.hpp")).read()
    bound = float(re.search(r"constexpr double kLnMaxUlp = ([0-9.]+);", text).group(1))
    log = open(os.path.join(ROOT, "profiles", "ln_sweep.log")).read()
    worst = float(re.search(r"worst error\s+([0-9.]+) ulp", log).group(1))
    assert int(re.search(r"inputs\s+(\d+)", log).group(1)) == 0x7f800000 - 1
    assert int(re.search(r"neighbours out of order\s+(\d+)", log).group(1)) == 0
    assert "ln sweep ok" in log
    assert worst <= bound < worst + 0.05 and abs(bound / 0.05 - round(bound / 0.05)) < 1e-9


def test_the_kernel_file_is_built_without_flush_to_zero_or_fast_math_and_without_contraction():
    mk = open(os.path.join(ROOT, "fast-dnn_amd", "csrc", "Makefile")).read()
    for flag in ("-ffast-math", "-fgpu-flush-denormals-to-zero", "-funsafe-math-optimizations", "-fdenormal-fp-math", "-Ofast", "-fassociative-math"):
        assert flag not in mk, flag
    assert "-ffp-contract=off" in mk and "fdnn_loglik.o" in mk


def test_ln_ref_specials_and_float64():
    x = TC.SPECIALS.copy()
    with np.errstate(all="ignore"):
        got = api.ln_ref(x)
        neg = (x.view(np.uint32) >> 31).astype(bool) & (x != 0)
        assert np.isnan(got[np.isnan(x) | neg]).all()
        assert (got[x == 0] == -np.inf).all() and got[np.isposinf(x)][0] == np.inf
    fin = ~np.isnan(x) & ~neg & (x != 0) & ~np.isinf(x)
    exact = np.log(x[fin].astype(np.float64))
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    assert (np.abs(got[fin].astype(np.float64) - exact) <= 0.85 * 2 * ulp).all()  # (np.spacing of the rounded value: at most twice the binade's ulp)
    assert api.ln_ref(np.float32(1.0)).view(np.uint32) == 0
    assert api.ln_ref(np.zeros((2, 3), np.float32)).shape == (2, 3)


def test_the_byte_comparison_is_not_blind():
    """On the binade [1/2, 1) the contract's ln differs from the correctly rounded float64 logarithm: a kernel that used
    another logarithm -- the hardware's, a library's -- would be caught by the byte comparison.  (The count is in DESIGN.md.)"""
    x = np.arange(0x3f000000, 0x3f800000, dtype=np.uint32).view(np.float32)
    got = api.ln_ref(x)
    rounded = np.log(x.astype(np.float64)).astype(np.float32)
    differ = int((got.view(np.uint32) != rounded.view(np.uint32)).sum())
    print(f"[1/2, 1): {differ} of {x.size} results differ from float32(log(float64(x)))")
    assert differ >= 1
    assert (np.diff(got) >= 0).all()  # monotone on the whole binade
    err = np.abs(got.astype(np.float64) - np.log(x.astype(np.float64))) / np.spacing(np.abs(rounded)).astype(np.float64)
    assert float(err.max()) <= 2 * 0.85


@pytest.mark.parametrize("width", LC.WIDTHS)
def test_loglik_ref_is_the_numpy_rule(width):
    n = 9 if width <= 1001 else 3
    lp = LC.priors(width)
    for kind in LC.ROW_KINDS:
        rows = LC.rows_of(kind, n, width)
        before = rows.view(np.uint32).copy()
        for floor in LC.FLOORS:
            for t in LC.TYPES:
                got = api.loglik_ref(rows, lp, floor, t)
                assert got.dtype == (np.float16 if t == api.LOGLIK_F16 else np.float32) and got.shape == rows.shape
                assert LC.same_bytes(got, LC.loglik_numpy(rows, lp, floor, t)), (kind, floor, t)
                if np.isfinite(floor):
                    assert not np.isneginf(got).any()  # with a finite floor no -inf leaves
                    assert (got[~np.isnan(got)] >= floor).all()
        assert np.array_equal(rows.view(np.uint32), before)


def test_fp16_keeps_what_fp16_probabilities_lose():
    p = np.array([[1e-9, 1e-30, 1.0, 0.5]], np.float32)
    lp = np.zeros(4, np.float32)
    got = api.loglik_ref(p, lp, -np.inf, api.LOGLIK_F16)
    assert p.astype(np.float16)[0, 0] == 0 and abs(float(got[0, 0]) + 20.72) < 0.02 and abs(float(got[0, 1]) + 69.08) < 0.05
    assert got[0, 2] == 0 and abs(float(got[0, 3]) + 0.6931) < 1e-3


def test_fp16_overflow_and_denormals():
    lp = np.array([-65504.0, -65519.9, -65520.0, 70000.0, 0.0, 0.0], np.float32)
    p = np.array([[1.0, 1.0, 1.0, 1.0, np.exp(np.float32(6e-8)), 1.0]], np.float32)
    got = api.loglik_ref(p, lp, -np.inf, api.LOGLIK_F16)
    assert got[0, 0] == np.float16(65504) and got[0, 1] == np.float16(65504) and np.isposinf(got[0, 2]) and np.isneginf(got[0, 3])
    s = api.loglik_ref(p, lp, -np.inf, api.LOGLIK_F32)
    assert LC.same_bytes(got, s.astype(np.float16))


def test_entries_ref_is_the_numpy_rule():
    width = 251
    lp = LC.priors(width)
    rng = np.random.default_rng(4)
    nodes = rng.integers(0, width, 1000).astype(np.int32)
    nodes[[3, 500, 999]] = (-1, width, np.iinfo(np.int32).min)
    p = LC.rows_of("softmax", 4, 250).ravel()
    p[:TC.SPECIALS.size] = TC.SPECIALS
    for floor in LC.FLOORS:
        for t in LC.TYPES:
            got = api.loglik_entries_ref(nodes, p, lp, floor, t)
            assert LC.same_bytes(got, LC.entries_numpy(nodes, p, lp, floor, t)), (floor, t)
            assert np.isnan(got[[3, 500, 999]]).all()


@pytest.mark.parametrize("lp,floor,t", [([0.0, np.inf], -np.inf, 0), ([np.nan, 0.0], -np.inf, 0), ([0.0, -np.inf], -np.inf, 1), ([0.0, 0.0], np.nan, 0),
                                        ([0.0, 0.0], np.inf, 0), ([0.0, 0.0], -65505.0, 1), ([0.0, 0.0], -1.0, 2), ([0.0, 0.0], -1.0, -1)])
def test_loglik_ref_refuses_bad_handles(lp, floor, t):
    with pytest.raises(api.FdnnError) as e:
        api.loglik_ref(np.ones((2, 2), np.float32), np.array(lp, np.float32), floor, t)
    assert e.value.code == api.FDNN_E_ARG


def test_a_floor_of_minus_65504_and_below_for_f32_are_fine():
    one = np.ones((1, 2), np.float32)
    assert api.loglik_ref(one, np.zeros(2, np.float32), -65504.0, api.LOGLIK_F16).dtype == np.float16
    assert api.loglik_ref(one, np.zeros(2, np.float32), -1e30, api.LOGLIK_F32).dtype == np.float32
