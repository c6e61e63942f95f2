"""The frames-form kernels alone (fdnn_fb_frames_rows_device) on planted device rows: frame_total and alpha_out are the BYTES
of the host restatement (api.fb_frames_ref, held to float64 by tests/test_fb_frames_host.py) with the start anchored and
free, in both forced forms and under the rule, uncut and cut at T / 2 with the carry row handed on, at the lane-block edges of
the wave form, on both sides of its limit and of the total's 256 partials, at the most states, at the edge of the arc-staging
cap, over 1 .. 65 segments, with guard words around frame_total, alpha_out and the scratch."""
import numpy as np
import pytest

import align_cases as AC
import align_graph_cases as GC
import loglik_cases as LL
from fast_dnn_amd import api
from test_gpu_fb_rows import GUARD, HANDLES, SCALE, WIDTH, Call, skip_chain

pytestmark = pytest.mark.gpu


class FramesCall(Call):
    def __init__(self):
        super().__init__()
        self.parts = []

    def add(self, rows, col, graph, node=None, gap=0):
        self.parts.append((np.ascontiguousarray(rows, np.float32), col, graph, node))
        return super().add(rows, col, graph, node, gap)

    def cut(self, second):
        """Every segment's rows before (or from) T / 2: the same graphs over half the frames."""
        c = FramesCall()
        for rows, col, graph, node in self.parts:
            c.add(rows[rows.shape[0] // 2:] if second else rows[:rows.shape[0] // 2], col, graph, node, gap=1)
        return c

    def ref(self, handle=None, lp=None, free=False, alpha_in=None):
        kw = dict(stateNode=self.node, log_prior=lp, floor=handle[0], type=handle[1]) if handle is not None else {}
        return api.fb_frames_ref(self.flat(), self.T, self.off, self.ld, api.pack_graphs(self.graphs), self.col, free_start=free, alpha_in=alpha_in, **kw)

    def device(self, torch, handle=None, lp=None, mode=0, free=False, alpha_in=None):
        """-> (frame_total, alpha_out, launches) of the call under kernel mode `mode`; the guard words are checked here."""
        api.set_fb_kernel(mode)
        try:
            ll = api.Loglik(lp, *handle) if handle is not None else None
            g = api.pack_graphs(self.graphs)
            dev = lambda a, ty: torch.from_numpy(np.ascontiguousarray(a, ty)).cuda()
            ptr = lambda d: d.data_ptr() if d is not None and d.numel() else 0
            d_rows, d_col, d_node = dev(self.flat(), np.float32), dev(self.col, np.int32), dev(self.node, np.int32)
            d_ap, d_src, d_lp = dev(g["arcPtr"], np.int32), dev(g["arcSrc"], np.int32), dev(g["arcLp"], np.float32)
            d_start = dev(g["startLp"], np.float32) if g["startLp"] is not None else None
            d_final = dev(g["finalLp"], np.float32) if g["finalLp"] is not None else None
            d_in = dev(alpha_in, np.float32) if alpha_in is not None else None
            words, n, rows = api.fb_frames_scratch_words(self.T, g["statePtr"]), len(self.col), int(np.sum(self.T))
            assert words == int((np.asarray(self.T, np.int64) * np.diff(g["statePtr"])).sum())
            d_scr = torch.full((words + 2 * GUARD,), -9.0, dtype=torch.float32, device="cuda")
            d_out = torch.full((n + 2 * GUARD,), -7.0, dtype=torch.float32, device="cuda")
            d_tot = torch.full((rows + 2 * GUARD,), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            before = api.fb_frames_launches()
            api.fb_frames_rows_device(ll, d_rows.data_ptr(), self.T, self.off, self.ld, g["statePtr"], g["arcPtr"], d_col.data_ptr(),
                                      d_node.data_ptr() if ll else 0, d_ap.data_ptr(), ptr(d_src), ptr(d_lp), ptr(d_start), ptr(d_final), free, ptr(d_in),
                                      d_out.data_ptr() + 4 * GUARD, d_scr.data_ptr() + 4 * GUARD, words, d_tot.data_ptr() + 4 * GUARD)
            torch.cuda.synchronize()
            after = api.fb_frames_launches()
            ao, ft = d_out.cpu().numpy(), d_tot.cpu().numpy()
            s = torch.cat([d_scr[:GUARD], d_scr[GUARD + words:]]).cpu().numpy()
            assert (ao[:GUARD] == -7).all() and (ao[GUARD + n:] == -7).all() and (ft[:GUARD] == -7).all() and (ft[GUARD + rows:] == -7).all() and (s == -9).all()
            if ll:
                ll.delete()
            return ft[GUARD:GUARD + rows], ao[GUARD:GUARD + n], tuple(b - a for a, b in zip(before, after))
        finally:
            api.set_fb_kernel(0)


def same(got, want):
    return all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got[:2], want))


def split(flat, Ts):
    return np.split(flat, np.cumsum(Ts)[:-1])


def held(torch, c, handle=None, lp=None, modes=((1, None), (2, (0, 1)), (0, None))):
    """The call anchored and free in every kernel mode, uncut and (its segments of two rows or more) cut at T / 2 with the
    device's own carry row, against the restatement -> the restatement's anchored and free frame_total.  The launch counts:
    `per` sweeps per form where given, and always one row-total launch per sweep launch."""
    both = []
    long = FramesCall()
    for part in c.parts:
        if part[0].shape[0] >= 2:
            long.add(*part, gap=1)
    for free in (False, True):
        want, want_long = c.ref(handle, lp, free), long.ref(handle, lp, free)
        both.append(want[0])
        for mode, per in modes:
            got = c.device(torch, handle, lp, mode, free)
            assert same(got, want), (free, mode, np.nonzero(got[0].view(np.uint32) != want[0].view(np.uint32))[0][:5])
            assert got[2][0] + got[2][1] == got[2][2] >= 1 and (per is None or got[2][:2] == per), (mode, got[2])
            a, b = long.cut(False), long.cut(True)
            first = a.device(torch, handle, lp, mode, free)
            second = b.device(torch, handle, lp, mode, free, alpha_in=first[1])
            joined = np.concatenate([x for pair in zip(split(first[0], a.T), split(second[0], b.T)) for x in pair])
            assert same((joined, second[1]), want_long), (free, mode, "cut")
    return both


SHAPES = (1, 2, 63, 64, 65, 255, 256, 257, 513, 1025)


def shapes_call(S, handle):
    """T = 1, 2, 5, 33 as four segments of one call: random graphs (in-degrees 0 .. 3, backward arcs, states without arcs,
    several start and final states) and, at T = 33, a skip chain whose first state is also a final state."""
    rng = np.random.default_rng(300 + S)
    c, ld = FramesCall(), 37
    for i, T in enumerate((1, 2, 5, 33)):
        rows = AC.probs(T, ld, 7 * S + i) if handle is not None else AC.scores(T, ld, 7 * S + i) * SCALE
        g = skip_chain(S, rng) if i == 3 else GC.random_graph(S, rng, starts=max(3, S // 4), finals=max(3, S // 4))
        if i == 3:
            g["final_lp"] = np.where(rng.random(S) < 0.5, np.log(rng.uniform(0.05, 0.95, S)), -np.inf).astype(np.float32)
            g["final_lp"][0] = 0.0
        c.add(rows, rng.integers(0, ld, S).tolist(), g, rng.integers(0, WIDTH, S).tolist(), gap=i)
    return c


@pytest.mark.parametrize("handle", HANDLES, ids=("scores", "f32", "f16"))
@pytest.mark.parametrize("S", SHAPES)
def test_shapes_in_every_form(S, handle):
    """T = 1 cannot be cut; the second half of T = 2 is a carried call of one row."""
    import torch

    wave = lambda limit: (1, 0) if S <= limit else (0, 1)
    anchored, free = held(torch, shapes_call(S, handle), handle, LL.priors(WIDTH), modes=((1, wave(256)), (2, (0, 1)), (0, wave(64))))
    assert not np.isnan(anchored).any() and not np.isnan(free).any() and (free >= anchored).all()


@pytest.mark.parametrize("what", ("most_states", 4095, 4097))
def test_the_most_states_and_the_arc_staging_cap(what):
    import torch

    rng = np.random.default_rng(5)
    if what == "most_states":  # S = 16384 at T = 2: the workgroup form, 64 states a partial of every row's total
        S = api.fb_limits()["max_states"]
        g = skip_chain(S, rng)
        g["start_lp"] = np.where(rng.random(S) < 0.5, 0.0, -np.inf).astype(np.float32)
        g["final_lp"] = np.log(rng.uniform(0.05, 0.95, S)).astype(np.float32)
        c = FramesCall().add(AC.scores(2, 8, 6) * SCALE, rng.integers(0, 8, S).tolist(), g)
        modes = ((0, (0, 1)),)
    else:  # one arc fewer and one more than the wave form stages in LDS, beside a small staged segment in the same launch
        S, arcs = 256, what
        deg = np.full(S, 16)
        deg[0] += arcs - 16 * S
        ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
        src = rng.integers(0, S, arcs).astype(np.int32)
        g = dict(states=np.zeros(S, np.int32), arc_ptr=ptr, arc_src=src, arc_lp=np.log(rng.uniform(0.05, 0.95, arcs)).astype(np.float32),
                 start_lp=np.log(rng.uniform(0.05, 0.95, S)).astype(np.float32), final_lp=np.zeros(S, np.float32))
        c = FramesCall().add(AC.scores(12, 23, 1) * SCALE, rng.integers(0, 23, S).tolist(), g).add(AC.scores(9, 23, 2) * SCALE, rng.integers(0, 23, 5).tolist(), skip_chain(5, rng))
        modes = ((1, (1, 0)), (2, (0, 1)), (0, (1, 1)))
    anchored, free = held(torch, c, modes=modes)
    assert np.isfinite(anchored[:c.T[0]]).all() and not np.isnan(anchored).any() and (free >= anchored).all() and (free != anchored).any()  # (the small chain's end is out of reach at its first frames: -inf)


@pytest.mark.parametrize("n_segs,launches", ((1, 1), (2, 1), (64, 1), (65, 2)))
def test_segments_per_launch(n_segs, launches):
    """Segments of unequal T and S inside the rule's wave form; 65 need a second sweep and a second row-total launch.  With a
    graph past the rule's limit beside them, one launch per form."""
    import torch

    rng = np.random.default_rng(20 + n_segs)
    c = FramesCall()
    for i in range(n_segs):
        S = int(rng.integers(1, 65))
        c.add(AC.scores(int(rng.integers(1, 40)), 11, 400 + i) * SCALE, rng.integers(0, 11, S).tolist(), skip_chain(S, rng) if i % 2 else GC.random_graph(S, rng),
              gap=int(rng.integers(0, 4)))
    for free in (False, True):
        got = c.device(torch, free=free)
        assert same(got, c.ref(free=free)) and got[2] == (launches, 0, launches)
    if n_segs == 2:
        c.add(AC.scores(70, 11, 600) * SCALE, rng.integers(0, 11, 300).tolist(), skip_chain(300, rng))
        got = c.device(torch, free=True)
        assert same(got, c.ref(free=True)) and got[2] == (1, 1, 2)


def test_argument_errors_launch_nothing():
    import torch

    before = api.fb_frames_launches()
    L, i32, i64 = api.lib(), api.C.POINTER(api.C.c_int), api.C.POINTER(api.C.c_longlong)
    buf = torch.zeros(1024, dtype=torch.float32, device="cuda")  # (the one call that launches reads 9 rows of 37 from it)
    p = buf.data_ptr()

    def call(T=(9,), off=(0,), ld=(37,), sp=(0, 5), ap=(0, 1, 2, 3, 4, 5), rows=p, col=p, d_ap=p, d_src=p, d_lp=p, free=0, a_in=None, a_out=p, scratch=p,
             words=45, total=p):
        a = [np.array(v, t) for v, t in ((T, np.int32), (off, np.int64), (ld, np.int32), (sp, np.int32))]
        h_ap = None if ap is None else np.array(ap, np.int32).ctypes.data_as(i32)
        return L.fdnn_fb_frames_rows_device(None, rows, a[0].ctypes.data_as(i32), a[1].ctypes.data_as(i64), a[2].ctypes.data_as(i32), a[3].ctypes.data_as(i32),
                                            h_ap, 1, col, None, d_ap, d_src, d_lp, None, None, free, a_in, a_out, scratch, words, total, None)

    for bad in (dict(T=(0,)), dict(ld=(0,)), dict(off=(-1,)), dict(sp=(0, 0)), dict(sp=(1, 6)), dict(sp=(0, 16385)), dict(rows=None), dict(col=None),
                dict(total=None), dict(rows=p + 2), dict(total=p + 2), dict(a_in=p + 2), dict(a_out=p + 2), dict(scratch=p + 2), dict(words=44),
                dict(scratch=None), dict(ap=None), dict(ap=(1, 1, 2, 3, 4, 5)), dict(ap=(0, 2, 1, 3, 4, 5)), dict(ap=tuple(np.arange(6) * 40000)),
                dict(d_ap=None), dict(d_src=None), dict(d_lp=None), dict(free=2), dict(free=-1)):
        assert call(**bad) == api.FDNN_E_ARG, bad
    with pytest.raises(api.FdnnError):
        api.fb_frames_scratch_words([16385], [0, 16384])  # the lattice is always needed: one row past the cap
    assert api.fb_frames_scratch_words([16384], [0, 16384]) == 1 << 28
    torch.cuda.synchronize()
    assert api.fb_frames_launches() == before
    assert call(a_out=None) == api.FDNN_OK  # the carry arrays are optional
    torch.cuda.synchronize()
    assert tuple(b - a for a, b in zip(before, api.fb_frames_launches())) == (1, 0, 1)
