"""Alignment graphs (the best path over any arc set of a segment's states), the half that needs no GPU: the stand-alone checker
of fdnn_align_graph.hpp under the sanitizers, the host restatement (api.align_graph_ref) against the recursion stated in numpy
(tests/align_graph_cases.py), the three graph builders against hand-written tables, the conditions that keep the byte
comparison from being blind, and that the new entry points are declared, exported and bound."""
import os
import subprocess

import numpy as np
import pytest

import align_cases as AC
import align_graph_cases as GC
import loglik_cases as LL
from conftest import ROOT
from fast_dnn_amd import api

INT_NAMES = ("fdnn_align_graph_rows_device", "fdnn_align_graph_scratch_words", "fdnn_ctx_align_graph", "fdnn_ctx_align_graph_device",
             "fdnn_calculate_align_graph", "fdnn_calculate_align_graph_raw", "fdnn_debug_align_graph_launches", "fdnn_debug_set_align_graph_kernel",
             "fdnn_debug_align_graph_limits", "fdnn_debug_align_graph_ref")


def host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    clang = os.path.join(rocm, "llvm", "bin", "clang++")
    return clang if os.path.exists(clang) else "g++"


def test_align_graph_header_and_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "align_graph_check")
    src = os.path.join(ROOT, "tests", "host", "align_graph_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    for line in ("align graph ok", "ref against brute force", "chain graphs against align::ref", "validator ok", "plan ok"):
        assert line in run.stdout, line


def test_align_graph_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fdnn.h")).read()
    for name in INT_NAMES:
        assert name in api.SIGNATURES and hasattr(api.lib(), name) and "FDNN_API int " + name + "(" in header, name
        at = header.index("FDNN_API int " + name + "(")
        assert "dnn.cc:355-392" in header[at - 9000:at], name  # cited as an extension of LazyOutputActivations
    assert "fdnn_align_graph.hpp" in header  # the contract is stated once, there
    for cls, methods in ((api.QuantizedDnn, ("calculateAlignGraph", "calculateAlignGraphRaw")), (api.LazyContext, ("alignGraph", "alignGraphDevice"))):
        for m in methods:
            assert callable(getattr(cls, m)), m
    for fn in ("align_graph_rows_device", "align_graph_ref", "align_graph_scratch_words", "align_graph_launches", "set_align_graph_kernel",
               "align_graph_limits", "chain_graph", "optional_silence_graph", "pack_graphs"):
        assert callable(getattr(api, fn)), fn
    assert len(api.align_graph_launches()) == 2
    assert not any("graph" in n for n in api.launch_names())  # counted apart from the recorder's table (fdnn_note.hpp)
    with pytest.raises(api.FdnnError):
        api.set_align_graph_kernel(3)
    api.set_align_graph_kernel(0)
    lim = api.align_graph_limits()
    assert lim == dict(max_states=16384, segs_per_launch=64, wave_states=256, max_arcs=1 << 17, lds_arcs=4096, lds_bp_words=4096, scratch_cap_mib=1024, wave_rule_states=64)


def test_the_kernel_file_is_built_without_fast_math_and_takes_its_arithmetic_from_the_headers():
    mk = open(os.path.join(ROOT, "fast-dnn_amd", "csrc", "Makefile")).read()
    assert "-ffp-contract=off" in mk and "fdnn_align_graph.o" in mk and "fdnn_align_graph.hpp" in mk
    src = open(os.path.join(ROOT, "fast-dnn_amd", "csrc", "fdnn_align_graph.hip")).read()
    for word in ("asm", "atomicAdd", "atomicCAS", "atomicMax", "fmaxf", "__device__ float g_", "__device__ int g_"):
        assert word not in src.replace("no inline assembly", ""), word
    for word in ("relax(", "better_end(", "align::emission(", "align::total_bits("):
        assert word in src, word
    hdr = open(os.path.join(ROOT, "fast-dnn_amd", "csrc", "fdnn_align_graph.hpp")).read()
    for word in ("build_sets(", "float emission(", "uint32_t total_bits(", "bool finite_bits("):  # reused, not restated
        assert word not in hdr, word


# ---------------------------------------------------------------- the builders against hand-written tables
def test_chain_graph_by_hand():
    g = api.chain_graph([7, 7, 3], self_lp=[-1, -2, -3], next_lp=[-10, -20, -30])
    assert g["states"].tolist() == [7, 7, 3] and g["arc_ptr"].tolist() == [0, 1, 3, 5]
    assert g["arc_src"].tolist() == [0, 1, 0, 2, 1] and g["arc_lp"].tolist() == [-1, -2, -10, -3, -20]  # self first, then the move
    assert g["start_lp"] is None and g["final_lp"] is None
    one = api.chain_graph([4])
    assert one["arc_ptr"].tolist() == [0, 1] and one["arc_src"].tolist() == [0] and one["arc_lp"].tolist() == [0]


def test_optional_silence_graph_by_hand():
    g = api.optional_silence_graph([[5, 6], [9]], 0, self_lp=-1, next_lp=-2, sil_self_lp=-3, enter_sil_lp=-4, leave_sil_lp=-5, skip_sil_lp=-6)
    #            sil0  5     6     sil3  9        sil5
    assert g["states"].tolist() == [0, 5, 6, 0, 9, 0]
    assert g["arc_ptr"].tolist() == [0, 1, 3, 5, 7, 10, 12]
    assert g["arc_src"].tolist() == [0, 1, 0, 2, 1, 3, 2, 4, 2, 3, 5, 4]
    assert g["arc_lp"].tolist() == [-3, -1, -5, -1, -2, -3, -4, -1, -6, -5, -3, -4]  # word 1's first state: the word before, then the silence
    assert g["start_lp"].tolist() == [0, 0, -np.inf, -np.inf, -np.inf, -np.inf]
    assert g["final_lp"].tolist() == [-np.inf, -np.inf, -np.inf, -np.inf, 0, 0]
    assert api.align_graph_limits()["max_states"] >= 6


def test_pack_graphs_by_hand():
    a = api.chain_graph([1, 2])
    b = api.optional_silence_graph([[3]], 0)
    p = api.pack_graphs([a, b, a])
    assert p["statePtr"].tolist() == [0, 2, 5, 7] and p["states"].tolist() == [1, 2, 0, 3, 0, 1, 2]
    assert p["arcPtr"].tolist() == [0, 1, 3, 4, 6, 8, 9, 11]          # global
    assert p["arcSrc"].tolist() == [0, 1, 0, 0, 1, 0, 2, 1, 0, 1, 0]  # local to each segment
    inf = np.inf
    assert p["startLp"].tolist() == [0, -inf, 0, 0, -inf, 0, -inf] and p["finalLp"].tolist() == [-inf, 0, -inf, 0, 0, -inf, 0]  # defaults written out
    q = api.pack_graphs([a, a])
    assert q["startLp"] is None and q["finalLp"] is None and q["arcPtr"].tolist() == [0, 1, 3, 4, 6]
    with pytest.raises(ValueError):
        api.pack_graphs([dict(a, arc_ptr=[0, 1])])


# ---------------------------------------------------------------- the restatement against numpy
@pytest.mark.parametrize("T,S", ((1, 1), (2, 1), (2, 2), (5, 5), (17, 4), (64, 33), (130, 40), (3, 40)))
def test_align_graph_ref_is_the_numpy_recursion(T, S):
    ld = max(3, S // 2)
    for seed in range(3):
        rng = np.random.default_rng(1000 * T + 10 * S + seed)
        col = rng.integers(0, ld, S)
        for kind in ("scores", "integers", "f32", "f16"):
            g = GC.random_graph(S, rng, integers=kind == "integers")
            if kind == "integers":  # planted ties
                rows = rng.integers(-3, 4, (T, ld)).astype(np.float32)
                got, want = GC.ref_one(rows, col, g), GC.graph_numpy(rows[:, col], g)
            elif kind == "scores":
                rows = AC.scores(T, ld, seed)
                before = rows.view(np.uint32).copy()
                got, want = GC.ref_one(rows, col, g), GC.graph_numpy(rows[:, col], g)
                assert np.array_equal(rows.view(np.uint32), before)
            else:
                t = api.LOGLIK_F16 if kind == "f16" else api.LOGLIK_F32
                rows, lp = AC.probs(T, ld, seed), LL.priors(11)
                node = rng.integers(0, 11, S)
                got = GC.ref_one(rows, col, g, stateNode=node, log_prior=lp, floor=-20.0, type=t)
                e = api.loglik_entries_ref(np.tile(node, T), rows[:, col].ravel(), lp, -20.0, t).astype(np.float32).reshape(T, S)
                want = GC.graph_numpy(e, g)
            assert np.array_equal(got[0], want[0]) and got[1].view(np.uint32)[0] == want[1], (kind, seed)


def test_the_chain_graph_gives_the_chain_restatements_bytes():
    for T, S in ((1, 1), (5, 5), (40, 12), (130, 40), (3, 5)):
        for seed in range(3):
            sl, nl = AC.transitions(S, seed)
            for rows in (AC.scores(T, S, seed), np.random.default_rng(seed).integers(-3, 4, (T, S)).astype(np.float32)):
                col = list(range(S))
                want = AC.one_segment(rows, col, selfLp=sl, nextLp=nl)
                got = GC.ref_one(rows, col, api.chain_graph(col, sl, nl))
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (T, S, seed)
                if T < S:
                    assert (got[0] == -1).all() and np.isneginf(got[1][0])


def test_several_segments_are_each_their_own_call():
    rng = np.random.default_rng(4)
    a, b = AC.scores(20, 7, 1), AC.scores(9, 5, 2)
    ga, gb = GC.random_graph(4, rng), GC.random_graph(3, rng)
    flat = np.concatenate([np.full(3, np.nan, np.float32), a.ravel(), np.full(2, np.nan, np.float32), b.ravel()])
    col = [0, 6, 6, 2, 4, 4, 0]
    path, total = api.align_graph_ref(flat, [20, 9], [3, 3 + a.size + 2], [7, 5], api.pack_graphs([ga, gb]), col)
    pa, ta = GC.ref_one(a, col[:4], ga)
    pb, tb = GC.ref_one(b, col[4:], gb)
    assert np.array_equal(path, np.concatenate([pa, pb])) and np.array_equal(total.view(np.uint32), np.concatenate([ta, tb]).view(np.uint32))


def test_out_of_range_values_are_nans_that_are_never_taken():
    rows = AC.scores(9, 4, 2)
    g = api.chain_graph([0, 0, 0, 0])
    ok = GC.ref_one(rows, [0, 1, 2, 3], g)
    assert np.isfinite(ok[1][0])
    for col in ([0, 1, 2, 4], [0, -1, 2, 3]):  # a column at the row stride; a negative one: no path, -inf -- never a NaN
        got = GC.ref_one(rows, col, g)
        assert (got[0] == -1).all() and np.isneginf(got[1][0])
    bad = dict(g, arc_src=np.array([0, 1, 9, 2, 1, 3, 2], np.int32))  # state 1's move comes from a source outside [0, S)
    got = GC.ref_one(rows, [0, 1, 2, 3], bad)
    assert (got[0] == -1).all() and np.isneginf(got[1][0])


# ---------------------------------------------------------------- the comparison is not blind
SEEDS = range(5)


def test_the_comparison_is_not_blind_on_optional_silence():
    """Conditions on the restatement alone, on 6 words x 6 states + 7 silences (S = 43, T = 129), scores 3 N(0, 1) - 5 over 64
    columns, silence in column 0, arc scores ln U(0.05, 0.95).  Observed with this generator, seeds 0 - 4: the best paths
    visit 22 of the 35 optional silences (3 - 6 of 7 per seed: 5, 3, 6, 4, 4); the path starts in the first word on seeds
    0, 1 and in the leading silence on seeds 2, 3, 4; it ends in the trailing silence on seeds 0, 2 and in the last word on
    seeds 1, 3, 4."""
    taken, starts, ends = [], set(), set()
    for seed in SEEDS:
        rows, g, col = GC.silence_case(seed)
        path, total = GC.ref_one(rows, col, g)
        want = GC.graph_numpy(rows[:, col], g)
        assert np.array_equal(path, want[0]) and total.view(np.uint32)[0] == want[1] and np.isfinite(total[0])
        sil = GC.silence_states(g)
        assert sil.size == 7 and col.size == 43
        seen = [int(s) for s in sil if (path == s).any()]
        taken.append(len(seen))
        starts.add(int(path[0])), ends.add(int(path[-1]))
        print(f"seed {seed}: {len(seen)} of 7 silences taken, starts in {path[0]}, ends in {path[-1]}")
    print("silences taken per seed:", taken)
    assert min(taken) >= 1 and sum(taken) < 7 * len(taken) and max(7 - t for t in taken) >= 1  # some taken, some skipped
    assert starts == {0, 1} and ends == {41, 42}  # both start and both final states are seen


@pytest.mark.parametrize("seed", SEEDS)
def test_the_arc_order_decides_ties(seed):
    """The scores rounded to integers and zero arc scores: reversing every state's arc order gives another path at an equal
    total.  Observed with this generator: 2 - 39 % of the frames change (seeds 0 - 4: 2, 7, 16, 3, 39 %)."""
    rows, g, col = GC.silence_case(seed, integers=True)
    a = GC.ref_one(rows, col, g)
    b = GC.ref_one(rows, col, GC.reversed_arcs(g))
    want = GC.graph_numpy(rows[:, col], GC.reversed_arcs(g))
    assert np.array_equal(b[0], want[0]) and b[1].view(np.uint32)[0] == want[1]
    frac = AC.differ(a[0], b[0])
    print(f"seed {seed}: reversing the arc order changes {frac:.0%} of the frames")
    assert a[1].view(np.uint32)[0] == b[1].view(np.uint32)[0] and np.isfinite(a[1][0]) and frac > 0
