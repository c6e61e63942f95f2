"""The frames-form best-path kernels alone (fdnn_align_frames_rows_device) against the host restatement (api.align_frames_ref,
held by tests/host/align_frames_check.cpp): the three per-frame arrays and begin_out byte for byte, d_out too except that a
NaN need only be a NaN -- every kernel body, modes 0, 1 and 2 with the launch counts, uncut and cut with the device's own carry."""
import numpy as np
import pytest

import align_cases as AC
import align_graph_cases as GC
import loglik_cases as LL
from fast_dnn_amd import api

pytestmark = pytest.mark.gpu
WIDTH, LD = 67, 23
HANDLES = (None, (-np.inf, api.LOGLIK_F32), (-20.0, api.LOGLIK_F16))
TS = (1, 9, 17, 18, 35)  # the group edges at 16 frames in flight
BODIES = {5: "wave k1", 64: "wave k1 full", 65: "wave k2", 130: "wave k4", 256: "wave k4, unstaged arcs", 300: "workgroup"}


def segment(S, T, seed, handle=None, base=0):
    """Random arcs (in-degree up to 3; up to 40 at S = 256: more than the wave form stages), half of the states start and final states."""
    rng = np.random.default_rng(seed)
    g = GC.random_graph(S, rng, max_deg=40 if S == 256 else 3, starts=max(2, S // 2), finals=max(2, S // 2))
    for key in ("start_lp", "final_lp"):
        g[key] = np.where(np.isfinite(g[key]), np.log(rng.uniform(0.05, 0.95, S)), -np.inf).astype(np.float32)
    rows = AC.probs(T, LD, seed) if handle is not None else AC.scores(T, LD, seed) * np.float32(0.2)
    return dict(rows=np.ascontiguousarray(rows, np.float32), col=rng.integers(0, LD, S), node=rng.integers(0, WIDTH, S), graph=g, device_graph=g, base=base)


def cut(segs, at, second):
    return [dict(s, rows=s["rows"][at(len(s["rows"])):] if second else s["rows"][:at(len(s["rows"]))], base=s["base"] + (at(len(s["rows"])) if second else 0))
            for s in segs]


def tables(segs, key="graph"):
    flat = np.concatenate([s["rows"].ravel() for s in segs])
    off = np.concatenate([[0], np.cumsum([s["rows"].size for s in segs])[:-1]])
    cat = lambda k: np.concatenate([s[k] for s in segs]).astype(np.int32)
    return flat, [len(s["rows"]) for s in segs], off, [LD] * len(segs), cat("col"), cat("node"), api.pack_graphs([s[key] for s in segs]), [s["base"] for s in segs]


def ref(segs, handle, free, carry=None):
    flat, T, off, ld, col, node, g, base = tables(segs, "device_graph")
    kw = dict(stateNode=node, log_prior=LL.priors(WIDTH), floor=handle[0], type=handle[1]) if handle is not None else {}
    best, end, begin, (d, b) = api.align_frames_ref(flat, T, off, ld, g, col, free_start=free, frame_base=base, carry=carry, **kw)
    return best, end, begin, d, b


def device(torch, segs, handle, mode, free, carry=None, in_place=False):
    """-> (frame_best, frame_end, frame_begin, d_out, begin_out, launches); in_place: each carry array is ONE buffer, in and out."""
    flat, T, off, ld, col, node, host, base = tables(segs)
    g = tables(segs, "device_graph")[6]
    dev = lambda a, ty: torch.from_numpy(np.ascontiguousarray(a, ty)).cuda()
    ins = [dev(flat, np.float32), dev(col, np.int32), dev(node, np.int32), dev(g["arcPtr"], np.int32), dev(g["arcSrc"], np.int32)]
    ins += [dev(g[k], np.float32) for k in ("arcLp", "startLp", "finalLp")]
    n, rows = col.size, int(np.sum(T))
    outs = [torch.full((size,), -7, dtype=ty, device="cuda") for size, ty in ((rows, torch.float32), (rows, torch.int32), (rows, torch.int32),
                                                                              (n, torch.float32), (n, torch.int32))]
    keep = [dev(a, a.dtype) for a in carry or ()]
    if in_place:
        outs[3].copy_(keep[0]), outs[4].copy_(keep[1])
        keep = outs[3:]
    p = [b.data_ptr() for b in ins]
    ll = api.Loglik(LL.priors(WIDTH), *handle) if handle is not None else None
    api.set_align_graph_kernel(mode)
    try:
        torch.cuda.synchronize()
        before = api.align_frames_launches()
        api.align_frames_rows_device(ll, p[0], T, off, ld, host["statePtr"], host["arcPtr"], p[1], p[2] if ll else 0, *p[3:], free, base,
                                     *([k.data_ptr() for k in keep] or [0, 0]), *[outs[i].data_ptr() for i in (3, 4, 0, 1, 2)])
        torch.cuda.synchronize()
    finally:
        api.set_align_graph_kernel(0)
        if ll:
            ll.delete()
    return tuple(o.cpu().numpy() for o in outs) + (tuple(y - x for x, y in zip(before, api.align_frames_launches())),)


def same(got, want):
    best, end, begin, d, b = want
    nan = np.isnan(d)
    return bool(not np.isnan(best).any() and np.array_equal(got[0].view(np.uint32), best.view(np.uint32)) and np.array_equal(got[1], end)
                and np.array_equal(got[2], begin) and np.array_equal(got[4], b) and np.array_equal(np.isnan(got[3]), nan)
                and np.array_equal(got[3].view(np.uint32)[~nan], d.view(np.uint32)[~nan]))


def held(torch, segs, handle, modes, carry=None, cuts=(lambda T: 1, lambda T: T // 2, lambda T: T - 1)):
    """Anchored and free, every mode, uncut and (segments of two rows or more) cut, the second cut in place -> the restatement's results."""
    long = [s for s in segs if len(s["rows"]) >= 2]
    both = []
    for free in (False, True):
        want, want_long = ref(segs, handle, free, carry), ref(long, handle, free, carry)
        both.append(want)
        for mode, launches in modes:
            got = device(torch, segs, handle, mode, free, carry)
            assert same(got, want) and got[5] == launches, (free, mode, got[5])
            for i, at in enumerate(cuts):
                a, b = cut(long, at, False), cut(long, at, True)
                first = device(torch, a, handle, mode, free, carry)
                second = device(torch, b, handle, mode, free, first[3:5], in_place=i == 1)
                split = lambda x, part: np.split(x, np.cumsum([len(s["rows"]) for s in part])[:-1])
                joined = tuple(np.concatenate([x for pair in zip(split(first[k], a), split(second[k], b)) for x in pair]) for k in range(3))
                assert same(joined + second[3:5], want_long), (free, mode, "cut", i)
    return both


@pytest.mark.parametrize("handle", HANDLES, ids=("scores", "f32", "f16"))
@pytest.mark.parametrize("S", list(BODIES), ids=list(BODIES.values()))
def test_every_kernel_body_at_the_group_edges(S, handle):
    import torch

    segs = [segment(S, T, 40 + 7 * i + S, handle, base=1000 * (i + 1)) for i, T in enumerate(TS)]
    assert S != 256 or len(segs[0]["graph"]["arc_src"]) > api.align_graph_limits()["lds_arcs"]
    wave = lambda limit: (1, 0) if S <= limit else (0, 1)
    anchored, free = held(torch, segs, handle, modes=((1, wave(256)), (2, (0, 1)), (0, wave(64))))
    assert (free[0] >= anchored[0]).all() and (handle is not None or (free[0] != anchored[0]).any())  # (d); not blind where a frame costs more than a start


@pytest.mark.parametrize("n_segs,launches", ((1, 1), (3, 1), (65, 2)))
def test_segments_per_launch(n_segs, launches):
    import torch

    rng = np.random.default_rng(20 + n_segs)
    segs = [segment(int(rng.integers(1, 65)), int(rng.integers(2, 40)), 400 + i, base=int(rng.integers(-5, 5000))) for i in range(n_segs)]
    held(torch, segs, None, modes=((0, (launches, 0)), (2, (0, launches))), cuts=(lambda T: T // 2, lambda T: T // 2))


def test_planted_bad_input():
    """One plant each beside a clean segment: a NaN column, a +inf frame, device arc sources outside [0, S), and a NaN in d_in."""
    import torch

    rng = np.random.default_rng(9)
    segs = [segment(64, 20, 900 + i, base=50 * i) for i in range(5)]
    segs[1]["rows"][3:, segs[1]["col"][32]] = np.nan
    segs[2]["rows"][17, :] = np.inf
    src = np.array(segs[3]["graph"]["arc_src"], np.int32)
    src[::7], src[3::7] = 64, -1
    segs[3]["device_graph"] = dict(segs[3]["graph"], arc_src=src)
    d = rng.uniform(-30, -5, 5 * 64).astype(np.float32)
    d[4 * 64 + int(np.argmax(d[4 * 64:]))] = np.nan
    for carry in (None, (d, rng.integers(-100, 100, d.size).astype(np.int32))):
        anchored, free = held(torch, segs, None, modes=((1, (1, 0)), (2, (0, 1))), carry=carry)
        assert not np.isnan(anchored[0]).any() and not np.isnan(free[0]).any() and np.isfinite(free[0][:20]).all()


def test_the_most_states_in_two_kernel_instances():
    """S = 8192, the limit: 128 KiB of LDS, asked for per kernel instance -- anchored, then free, in one process."""
    import torch

    held(torch, [segment(8192, 3, 77, base=5)], None, modes=((0, (0, 1)),), cuts=(lambda T: 1,))
    with pytest.raises(api.FdnnError):
        device(torch, [segment(8193, 1, 78)], None, 0, False)
