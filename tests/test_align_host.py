"""Forced alignment (the best monotone path of a transcript's states over an utterance's rows), the half that needs no GPU: the
stand-alone checker of fdnn_align.hpp under the sanitizers, the host restatement (api.align_ref) against the recursion stated
in numpy (tests/align_cases.py), the conditions that keep the byte comparison from being blind, and that the new entry points
are declared, exported and bound."""
import os
import subprocess

import numpy as np
import pytest

import align_cases as AC
import loglik_cases as LL
from conftest import ROOT
from fast_dnn_amd import api

INT_NAMES = ("fdnn_align_rows_device", "fdnn_align_scratch_words", "fdnn_ctx_align", "fdnn_ctx_align_device", "fdnn_calculate_align",
             "fdnn_calculate_align_raw", "fdnn_debug_align_launches", "fdnn_debug_set_align_kernel", "fdnn_debug_align_limits", "fdnn_debug_align_ref",
             "fdnn_debug_align_sets")


def host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    clang = os.path.join(rocm, "llvm", "bin", "clang++")
    return clang if os.path.exists(clang) else "g++"


def test_align_header_and_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "align_check")
    src = os.path.join(ROOT, "tests", "host", "align_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "align ok" in run.stdout and "ref against brute force" in run.stdout and "plan ok" in run.stdout


def test_align_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fdnn.h")).read()
    for name in INT_NAMES:
        assert name in api.SIGNATURES and hasattr(api.lib(), name) and "FDNN_API int " + name + "(" in header, name
        at = header.index("FDNN_API int " + name + "(")
        assert "dnn.cc:355-392" in header[at - 9000:at], name  # cited as an extension of LazyOutputActivations
    for cls, methods in ((api.QuantizedDnn, ("calculateAlign", "calculateAlignRaw")), (api.LazyContext, ("align", "alignDevice"))):
        for m in methods:
            assert callable(getattr(cls, m)), m
    for fn in ("align_rows_device", "align_ref", "align_sets", "align_launches", "set_align_kernel", "align_limits", "align_scratch_words"):
        assert callable(getattr(api, fn)), fn
    assert len(api.align_launches()) == 2
    assert not any(n.startswith("align") for n in api.launch_names())  # counted apart from the recorder's table (fdnn_note.hpp)
    with pytest.raises(api.FdnnError):
        api.set_align_kernel(3)
    api.set_align_kernel(0)
    lim = api.align_limits()
    assert lim["max_states"] == 16384 and lim["segs_per_launch"] == 64 and lim["wave_states"] == 1024 and lim["scratch_cap_mib"] == 1024


def test_the_kernel_file_is_built_without_flush_to_zero_or_fast_math_and_without_contraction():
    mk = open(os.path.join(ROOT, "fast-dnn_amd", "csrc", "Makefile")).read()
    for flag in ("-ffast-math", "-fgpu-flush-denormals-to-zero", "-funsafe-math-optimizations", "-fdenormal-fp-math", "-Ofast", "-fassociative-math"):
        assert flag not in mk, flag
    assert "-ffp-contract=off" in mk and "fdnn_align.o" in mk and "fdnn_align.hpp" in mk
    src = open(os.path.join(ROOT, "fast-dnn_amd", "csrc", "fdnn_align.hip")).read()
    for word in ("asm", "atomicAdd", "atomicCAS", "atomicMax", "fmaxf", "__device__ float g_", "__device__ int g_"):
        assert word not in src.replace("no inline assembly", ""), word


@pytest.mark.parametrize("T,S", ((1, 1), (2, 1), (2, 2), (5, 5), (17, 4), (64, 33), (130, 40), (130, 1), (40, 40)))
def test_align_ref_is_the_numpy_recursion(T, S):
    ld = max(3, S // 2)
    for seed in range(3):
        rng = np.random.default_rng(1000 * T + 10 * S + seed)
        col = rng.integers(0, ld, S)
        sl, nl = AC.transitions(S, seed)
        for kind in ("scores", "integers", "f32", "f16"):
            if kind == "integers":  # planted ties
                rows = rng.integers(-3, 4, (T, ld)).astype(np.float32)
                got = AC.one_segment(rows, col)
                want = AC.align_numpy(rows[:, col])
            elif kind == "scores":
                rows = AC.scores(T, ld, seed)
                before = rows.view(np.uint32).copy()
                got = AC.one_segment(rows, col, selfLp=sl, nextLp=nl)
                want = AC.align_numpy(rows[:, col], sl, nl)
                assert np.array_equal(rows.view(np.uint32), before)
            else:
                t = api.LOGLIK_F16 if kind == "f16" else api.LOGLIK_F32
                rows, lp = AC.probs(T, ld, seed), LL.priors(11)
                node = rng.integers(0, 11, S)
                got = AC.one_segment(rows, col, stateNode=node, log_prior=lp, floor=-20.0, type=t, selfLp=sl, nextLp=nl)
                e = api.loglik_entries_ref(np.tile(node, T), rows[:, col].ravel(), lp, -20.0, t).astype(np.float32).reshape(T, S)
                want = AC.align_numpy(e, sl, nl)
            assert np.array_equal(got[0], want[0]) and got[1].view(np.uint32)[0] == want[1], (kind, seed)
            assert got[0][0] == 0 and got[0][-1] == S - 1 and set(np.diff(got[0]).tolist()) <= {0, 1}


def test_several_segments_are_each_their_own_call():
    a, b = AC.scores(20, 7, 1), AC.scores(9, 5, 2)
    flat = np.concatenate([np.full(3, np.nan, np.float32), a.ravel(), np.full(2, np.nan, np.float32), b.ravel()])
    col = [0, 6, 6, 2, 4, 4, 0]
    sl, nl = AC.transitions(7, 3)
    path, total = api.align_ref(flat, [20, 9], [3, 3 + a.size + 2], [7, 5], [0, 4, 7], col, selfLp=sl, nextLp=nl)
    pa, ta = AC.one_segment(a, col[:4], selfLp=sl[:4], nextLp=nl[:4])
    pb, tb = AC.one_segment(b, col[4:], selfLp=sl[4:], nextLp=nl[4:])
    assert np.array_equal(path, np.concatenate([pa, pb])) and np.array_equal(total.view(np.uint32), np.concatenate([ta, tb]).view(np.uint32))


def test_non_finite_totals_give_minus_one_everywhere():
    short = AC.one_segment(AC.scores(3, 5, 1), list(range(5)))
    assert (short[0] == -1).all() and np.isneginf(short[1][0])
    rows = AC.scores(9, 4, 2)
    rows[4] = np.nan
    got = AC.one_segment(rows, list(range(4)))
    assert (got[0] == -1).all() and got[1].view(np.uint32)[0] == AC.QNAN
    want = AC.align_numpy(rows)
    assert (want[0] == -1).all() and want[1] == AC.QNAN
    zeros = AC.one_segment(np.zeros((12, 5), np.float32), list(range(5)))
    assert zeros[0].tolist() == [0, 1, 2, 3, 4] + [4] * 7 and zeros[1].view(np.uint32)[0] == 0


def test_align_sets_are_the_transcripts_distinct_nodes():
    sp = [0, 7, 10, 11]
    st = [9, 7, 7, 3, 9, 0, 3, 5, 5, 5, 2]
    set_ptr, nodes, col = api.align_sets(sp, st)
    assert set_ptr.tolist() == [0, 4, 5, 6] and nodes.tolist() == [0, 3, 7, 9, 5, 2]
    for s in range(3):
        for j in range(sp[s], sp[s + 1]):
            assert nodes[set_ptr[s] + col[j]] == st[j]
    assert api.sets_check([0, 5, 9, 12], set_ptr, nodes, 10, 12) == 0  # the form fdnn_calculate_lazy_sets takes


@pytest.mark.parametrize("seed", range(5))
def test_the_comparison_is_not_blind(seed):
    """Conditions on the restatement alone: on decoder-like scores the path depends on the transition scores and is far from
    the uniform segmentation -- a kernel that ignored either, or an off-by-one in the back-trace, would be caught."""
    T, S = 130, 40
    rows, sl, nl = AC.decoder_case(T, S, seed)
    col = list(range(S))
    with_t = AC.one_segment(rows, col, selfLp=sl, nextLp=nl)[0]
    without = AC.one_segment(rows, col)[0]
    a, b = AC.differ(with_t, without), AC.differ(with_t, AC.uniform_path(T, S))
    print(f"seed {seed}: with / without transitions differ in {a:.0%} of the frames, path / uniform segmentation in {b:.0%}")
    assert a >= 0.10 and b >= 0.50
