"""The frames form of the summed alignment graphs, the half that needs no GPU: the stand-alone checker of fdnn_fb_frames.hpp
under the sanitizers, the host restatement (api.fb_frames_ref) against a float64 numpy recursion under bound (e) of the
header, the new symbols, and the condition that keeps the GPU comparison from being blind."""
import os
import subprocess

import numpy as np
import pytest

import fb_cases as FC
from conftest import ROOT
from fast_dnn_amd import api
from test_fb_host import host_compiler
from test_gpu_fb_frames_rows import HANDLES, SHAPES, frames_of, plants, shapes_call

INT_NAMES = ("fdnn_fb_frames_rows_device", "fdnn_fb_frames_scratch_words", "fdnn_ctx_fb_frames", "fdnn_ctx_fb_frames_device", "fdnn_calculate_fb_frames",
             "fdnn_calculate_fb_frames_raw", "fdnn_debug_fb_frames_ref", "fdnn_debug_fb_frames_launches")


def test_fb_frames_header_and_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "fb_frames_check")
    src = os.path.join(ROOT, "tests", "host", "fb_frames_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run([host_compiler(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    for line in ("fb frames ok", "prefixes ok", "every cut ok", "never a NaN", "free start ok", "plan ok"):
        assert line in run.stdout, line


def test_fb_frames_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fdnn.h")).read()
    for name in INT_NAMES:
        assert name in api.SIGNATURES and hasattr(api.lib(), name) and "FDNN_API int " + name + "(" in header, name
    assert "fdnn_fb_frames.hpp" in header  # the contract is stated once, there
    for cls, methods in ((api.QuantizedDnn, ("calculateFbFrames", "calculateFbFramesRaw")), (api.LazyContext, ("fbFrames", "fbFramesDevice"))):
        for m in methods:
            assert callable(getattr(cls, m)), m
    for fn in ("fb_frames_rows_device", "fb_frames_ref", "fb_frames_launches", "fb_frames_scratch_words"):
        assert callable(getattr(api, fn)), fn
    assert len(api.fb_frames_launches()) == 3


def frames64(e, g, free, alpha_in=None):
    """The contract in float64 with numpy's logaddexp -> (frame_total [T], the header's M, A)."""
    e = np.asarray(e, np.float64)
    T, S = e.shape
    ptr, src, lp = np.asarray(g["arc_ptr"]), np.asarray(g["arc_src"]), np.asarray(g["arc_lp"], np.float64)
    dst = np.repeat(np.arange(S), np.diff(ptr))
    start, final = FC.ends(g)
    total, big = np.empty(T), [0.0]
    prev = None if alpha_in is None else np.asarray(alpha_in, np.float64)
    with np.errstate(all="ignore"):
        for t in range(T):
            if prev is None:
                acc = start.copy()
            else:
                acc = np.full(S, -np.inf)
                np.logaddexp.at(acc, dst, prev[src] + lp)
                acc = np.logaddexp(acc, start) if free else acc
            prev = acc + e[t]
            total[t] = np.logaddexp.reduce(prev + final)
            big.append(np.abs(prev[np.isfinite(prev)]).max(initial=0.0))
    step = max([np.abs(x[np.isfinite(x)]).max(initial=0.0) for x in (lp, final, start)])
    return total, max(big) + step, int(np.diff(ptr).max()) if S else 0


@pytest.mark.parametrize("free", (False, True))
@pytest.mark.parametrize("seed", range(3))
def test_fb_frames_ref_is_the_recursion_within_bound_e(seed, free):
    """(e): |frame_total[t] - total64[t]| <= delta_bound(t + 1, S, A + free_start, M), M and A the case's own."""
    rows, g, col = FC.soft_silence_case(seed)
    T, S, ld = rows.shape[0], col.size, rows.shape[1]
    packed = api.pack_graphs([g])
    got, _ = api.fb_frames_ref(rows, [T], [0], [ld], packed, col, free_start=free)
    want, M, A = frames64(rows[:, col], g, free)
    for t in range(T):
        bound = FC.delta_bound(t + 1, S, A + int(free), M)
        assert (got[t] == want[t]) if not np.isfinite(want[t]) else abs(float(got[t]) - want[t]) <= bound, (t, got[t], want[t], bound)
    assert np.isfinite(want).sum() > T // 2 and not np.isnan(got).any()
    if not free:  # (a): the last frame is the whole segment's total
        assert got.view(np.uint32)[-1] == FC.ref_one(rows, col, g, want_gamma=False)[0].view(np.uint32)[0]


@pytest.mark.parametrize("handle", HANDLES, ids=("scores", "f32", "f16"))
@pytest.mark.parametrize("S", SHAPES)
def test_the_gpu_cases_are_not_blind(S, handle):
    """A condition on the INPUTS of tests/test_gpu_fb_frames_rows.py, from the restatement alone, on the case's 33-frame segment:
    the free-start frame_total differs in bytes from the anchored one in at least half of the frames t >= 1 -- else a kernel
    that drops the start term would pass --, and the anchored frame_total is not constant over t -- else a kernel that
    repeats one total would."""
    from loglik_cases import priors

    c = shapes_call(S, handle)
    anchored, free = (c.ref(handle, priors(67), f)[0][-33:] for f in (False, True))
    assert (anchored.view(np.uint32)[1:] != free.view(np.uint32)[1:]).mean() >= 0.5
    assert np.unique(anchored.view(np.uint32)).size > 16 and np.isfinite(anchored).all()


def test_the_planted_cases_are_not_blind():
    """A condition on the planted INPUTS of tests/test_gpu_fb_frames_rows.py, from the restatement alone.  Every planted
    segment's frame_total differs in bytes, in a frame at or after the plant, from the same call with clean values in the
    planted ones' place, anchored and free alike -- else a kernel that ignored the plant would pass.  And over the whole file
    at least half of the planted segments, counted under either start, keep a finite frame_total at their last frame -- else
    most of the comparisons would be of -inf with -inf."""
    from loglik_cases import priors

    finite = total = 0
    for name, p in plants().items():
        lp = priors(67) if p.handle is not None else None
        assert p.at, name
        for free in (False, True):
            got = p.call.ref(p.handle, lp, free, p.alpha_in)[0].view(np.uint32)
            clean = p.clean.ref(p.handle, lp, free, p.clean_in)[0].view(np.uint32)
            assert not np.isnan(got.view(np.float32)).any() and np.isfinite(clean.view(np.float32)).all(), name
            for seg, t0 in p.at.items():
                frames = frames_of(p.call, seg)
                assert (got[frames][t0:] != clean[frames][t0:]).any(), (name, seg, free)
                assert np.array_equal(got[frames][:t0], clean[frames][:t0]), (name, seg, free)  # and in none before it
                finite += bool(np.isfinite(got.view(np.float32)[frames][-1]))
                total += 1
            first = frames_of(p.call, 0)
            assert 0 not in p.at and np.array_equal(got[first], clean[first]), (name, free)  # the clean segment is clean
    print(f"{finite} of {total} planted (segment, start) pairs end finite")
    assert 2 * finite >= total


def test_the_lower_clamp_of_the_device_arc_offsets_shows_in_the_bytes():
    """The planted device arc offset BELOW a segment's first arc, from the restatement alone (a kernel without the lower bound
    would read outside the segment's arcs, so no device run may try it).  Such a kernel steps state j over the arcs
    min(ptr[j], arcs) .. min(ptr[j + 1], arcs) of the call's table counted from the segment's first arc: the negative
    offset reaches the arcs of the segment BEFORE it.  The restatement over exactly those arcs differs in bytes from the
    restatement over clamped() in every planted segment, so the case holds the kernels to the lower bound too."""
    p = plants()["device arc offsets below and above the segment"]
    packed = api.pack_graphs(p.call.graphs)
    for seg in p.at:
        rows, col, g, _ = p.call.parts[seg]
        s0, S = int(packed["statePtr"][seg]), len(col)
        arc0, arcs = int(packed["arcPtr"][s0]), len(g["arc_src"])
        ptr = packed["arcPtr"][s0:s0 + S + 1].astype(np.int64) - arc0
        for at, value in p.call.device_ptr.items():
            if s0 <= at <= s0 + S:
                ptr[at - s0] = value - arc0
        assert ptr.min() < 0 and ptr.max() > arcs and arc0 + ptr.min() >= 0  # one below, one above, and inside the call's table
        q = np.minimum(ptr, arcs)  # the upper bound alone
        take = [arc0 + np.arange(q[j], max(q[j], q[j + 1])) for j in range(S)]
        at = np.concatenate(take).astype(np.int64)
        loose = dict(g, arc_ptr=np.concatenate([[0], np.cumsum([t.size for t in take])]).astype(np.int32), arc_src=packed["arcSrc"][at], arc_lp=packed["arcLp"][at])
        for free in (False, True):
            one = lambda graph: api.fb_frames_ref(rows, [rows.shape[0]], [0], [rows.shape[1]], api.pack_graphs([graph]), col, free_start=free)[0]
            want, without = one(p.call.ref_graphs[seg]), one(loose)
            assert not np.array_equal(want.view(np.uint32), without.view(np.uint32)), (seg, free)
            assert np.array_equal(want.view(np.uint32), p.call.ref(free=free)[0].view(np.uint32)[frames_of(p.call, seg)])  # (the case's own expectation)
