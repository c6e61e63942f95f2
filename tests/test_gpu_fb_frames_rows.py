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
        self.ref_graphs = None  # (what the restatement runs over where it is neither device_graphs nor the host tables)
        self.device_ptr = {}    # (index into the call's device arcPtr: the value planted there)

    def add(self, rows, col, graph, node=None, gap=0):
        self.parts.append((np.ascontiguousarray(rows, np.float32), col, graph, node))
        return super().add(rows, col, graph, node, gap)

    def cut(self, second):
        """Every segment's rows before (or from) T / 2: the same graphs over half the frames."""
        c = FramesCall()
        for rows, col, graph, node in self.parts:
            c.add(rows[rows.shape[0] // 2:] if second else rows[:rows.shape[0] // 2], col, graph, node, gap=1)
        c.device_graphs, c.ref_graphs, c.device_ptr = self.device_graphs, self.ref_graphs, self.device_ptr
        return c

    def ref(self, handle=None, lp=None, free=False, alpha_in=None):
        kw = dict(stateNode=self.node, log_prior=lp, floor=handle[0], type=handle[1]) if handle is not None else {}
        g = api.pack_graphs(self.ref_graphs or self.device_graphs or self.graphs)
        return api.fb_frames_ref(self.flat(), self.T, self.off, self.ld, g, self.col, free_start=free, alpha_in=alpha_in, **kw)

    def device(self, torch, handle=None, lp=None, mode=0, free=False, alpha_in=None, in_place=False):
        """-> (frame_total, alpha_out, launches) of the call under kernel mode `mode`; the guard words are checked here.  The
        HOST tables (the plan's) are always those of self.graphs; the device copies are device_graphs' with device_ptr's
        entries written over arcPtr.  in_place: alpha_in and alpha_out are ONE device buffer."""
        api.set_fb_kernel(mode)
        try:
            ll = api.Loglik(lp, *handle) if handle is not None else None
            host = api.pack_graphs(self.graphs)
            g = dict(api.pack_graphs(self.device_graphs or self.graphs))
            assert np.array_equal(g["statePtr"], host["statePtr"]) and g["arcSrc"].size == host["arcSrc"].size
            g["arcPtr"] = g["arcPtr"].copy()
            for at, value in self.device_ptr.items():
                g["arcPtr"][at] = value
            dev = lambda a, ty: torch.from_numpy(np.ascontiguousarray(a, ty)).cuda()
            ptr = lambda d: d.data_ptr() if d is not None and d.numel() else 0
            d_rows, d_col, d_node = dev(self.flat(), np.float32), dev(self.col, np.int32), dev(self.node, np.int32)
            d_ap, d_src, d_lp = dev(g["arcPtr"], np.int32), dev(g["arcSrc"], np.int32), dev(g["arcLp"], np.float32)
            d_start = dev(g["startLp"], np.float32) if g["startLp"] is not None else None
            d_final = dev(g["finalLp"], np.float32) if g["finalLp"] is not None else None
            d_in = dev(alpha_in, np.float32) if alpha_in is not None else None
            words, n, rows = api.fb_frames_scratch_words(self.T, host["statePtr"]), len(self.col), int(np.sum(self.T))
            assert words == int((np.asarray(self.T, np.int64) * np.diff(host["statePtr"])).sum())
            d_scr = torch.full((words + 2 * GUARD,), -9.0, dtype=torch.float32, device="cuda")
            d_out = torch.full((n + 2 * GUARD,), -7.0, dtype=torch.float32, device="cuda")
            if in_place:
                d_out[GUARD:GUARD + n] = d_in
                d_in = d_out[GUARD:GUARD + n]
            d_tot = torch.full((rows + 2 * GUARD,), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            before = api.fb_frames_launches()
            api.fb_frames_rows_device(ll, d_rows.data_ptr(), self.T, self.off, self.ld, host["statePtr"], host["arcPtr"], d_col.data_ptr(),
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


def same_but_nan(got, want):
    """The rule for planted input (fdnn_fb_frames.hpp, beside alpha_out): frame_total is never a NaN and is compared byte for
    byte; alpha_out byte for byte where the restatement's value is no NaN, and a NaN -- any payload, either sign: the host's
    and the device's inf - inf need not share a sign bit -- exactly where the restatement's is one."""
    nan = np.isnan(want[1])
    return bool(not np.isnan(want[0]).any() and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(np.isnan(got[1]), nan)
                and np.array_equal(got[1].view(np.uint32)[~nan], want[1].view(np.uint32)[~nan]))


def held(torch, c, handle=None, lp=None, modes=((1, None), (2, (0, 1)), (0, None)), alpha_in=None, equal=same):
    """The call anchored and free in every kernel mode, uncut and (its segments of two rows or more) cut at T / 2 with the
    device's own carry row, against the restatement -> the restatement's anchored and free frame_total.  The launch counts:
    `per` sweeps per form where given, and always one row-total launch per sweep launch.  alpha_in: the call itself is
    carried (then every segment has two rows or more, so the row is the cut call's too)."""
    both = []
    long = FramesCall()
    for part in c.parts:
        if part[0].shape[0] >= 2:
            long.add(*part, gap=1)
    long.device_graphs, long.ref_graphs, long.device_ptr = c.device_graphs, c.ref_graphs, c.device_ptr
    assert len(long.parts) == len(c.parts) or (alpha_in is None and c.device_graphs is None and c.ref_graphs is None and not c.device_ptr)
    for free in (False, True):
        want, want_long = c.ref(handle, lp, free, alpha_in), long.ref(handle, lp, free, alpha_in)
        both.append(want[0])
        for mode, per in modes:
            got = c.device(torch, handle, lp, mode, free, alpha_in)
            assert equal(got, want), (free, mode, np.nonzero(got[0].view(np.uint32) != want[0].view(np.uint32))[0][:5])
            assert got[2][0] + got[2][1] == got[2][2] >= 1 and (per is None or got[2][:2] == per), (mode, got[2])
            a, b = long.cut(False), long.cut(True)
            first = a.device(torch, handle, lp, mode, free, alpha_in)
            second = b.device(torch, handle, lp, mode, free, alpha_in=first[1])
            joined = np.concatenate([x for pair in zip(split(first[0], a.T), split(second[0], b.T)) for x in pair])
            assert equal((joined, second[1]), want_long), (free, mode, "cut")
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


# ------------------------------------------------------------------------------------------------ planted bad input
# Values the kernels must refuse or carry without a NaN in frame_total: every case is a Plant -- a call whose first segment
# is clean and whose others hold the planted values, and the same call with clean values in their place (for the
# condition in tests/test_fb_frames_host.py that keeps the cases from being blind).  Every planted index is one the kernels
# are written to refuse WITHOUT reading: nothing here reads outside a buffer.
FLOOR32, FLOOR16 = (-20.0, api.LOGLIK_F32), (-20.0, api.LOGLIK_F16)
AS_PROBS = (0.0, -0.25, np.nan, np.inf)  # under a handle: ln 0 is floored, ln of a negative value is a NaN
ARCS = "256 states, 4097 arcs"  # the unstaged wave segment
# (S, T, planted frame) by the kernel body the launch takes in mode 1.  frames_in_flight(1) = 16 and an uncarried sweep
# steps frames 1 ..: T = 17 is one full group (frames 3 and 16: its first and last quarter), T = 18 leaves frame 17 alone in
# a partial last group, T = 35 has frame 20 in a LATER full group (17 .. 32) and frame 33 in the partial last one; T = 9 is
# one partial group
GROUPS = {"k1": ((5, 9, 3), (64, 9, 3), (5, 17, 3), (64, 17, 16), (5, 18, 17), (64, 18, 17), (5, 35, 20), (64, 35, 20), (64, 35, 33)), "k2": ((65, 9, 3),),
          "k4": ((130, 9, 3), (ARCS, 9, 3)), "wg": ((300, 9, 3),)}
BAD_SOURCES = (None, -1, 1 << 16, -(1 << 31), 65535)  # None: the segment's own S.  65535 is the 16-bit staging's sentinel


def open_chain(S, rng):
    """A skip chain that may be entered and left in every state: a finite total at any T, and round any one state."""
    g = skip_chain(S, rng)
    g["start_lp"] = np.log(rng.uniform(0.05, 0.95, S)).astype(np.float32)
    g["final_lp"] = np.log(rng.uniform(0.05, 0.95, S)).astype(np.float32)
    return g


def many_arcs(rng, arcs=4097):
    """256 states, 16 arcs into each and the rest into state 0: one arc more than the wave form stages in LDS."""
    S = 256
    deg = np.full(S, 16)
    deg[0] += arcs - 16 * S
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    src = rng.integers(0, S, arcs).astype(np.int32)
    src[ptr[:-1]] = np.arange(S)  # a self-loop first
    return dict(states=np.zeros(S, np.int32), arc_ptr=ptr, arc_src=src, arc_lp=np.log(rng.uniform(0.05, 0.95, arcs)).astype(np.float32),
                start_lp=np.log(rng.uniform(0.05, 0.95, S)).astype(np.float32), final_lp=np.log(rng.uniform(0.05, 0.95, S)).astype(np.float32))


def segment(S, T, seed, handle=None):
    """-> (rows, col, graph, node): a column of its own for every state, so a planted column is one state's."""
    rng = np.random.default_rng(seed)
    g = many_arcs(rng) if S == ARCS else open_chain(S, rng)
    n = len(g["states"])
    ld = n + 3
    rows = AC.probs(T, ld, seed) if handle is not None else AC.scores(T, ld, seed) * SCALE
    return rows, rng.permutation(ld)[:n].tolist(), g, rng.integers(0, WIDTH, n).tolist()


def heavy(seg, t, handle=None):
    """The state with the largest term of frame t's total, from the restatement: a plant there shows in the total's bytes."""
    rows, col, g, node = seg
    kw = dict(stateNode=node, log_prior=LL.priors(WIDTH), floor=handle[0], type=handle[1]) if handle is not None else {}
    alpha = api.fb_frames_ref(rows[:t + 1], [t + 1], [0], [rows.shape[1]], api.pack_graphs([g]), col, **kw)[1]
    return int(np.argmax(alpha + g["final_lp"]))


def clamped(g, ptr):
    """The graph the kernels run where a segment's DEVICE arc offsets are `ptr` (local to the segment): every offset is
    clamped into [0, arcs of the HOST table], and state j takes the arcs clamp(ptr[j]) .. clamp(ptr[j + 1]) -- none where
    that range is empty or reversed --, whichever states the host table gives them to."""
    n = len(g["arc_src"])
    p = np.clip(np.asarray(ptr, np.int64), 0, n)
    take = [np.arange(p[j], max(p[j], p[j + 1])) for j in range(len(g["states"]))]
    at = np.concatenate(take).astype(np.int64)
    return dict(g, arc_ptr=np.concatenate([[0], np.cumsum([t.size for t in take])]).astype(np.int32), arc_src=np.asarray(g["arc_src"])[at],
                arc_lp=np.asarray(g["arc_lp"])[at])


class Plant:
    def __init__(self, handle=None):
        self.call, self.clean, self.at, self.handle = FramesCall(), FramesCall(), {}, handle
        self.dev, self.refg, self.alpha_in, self.clean_in = [], [], None, None

    def add(self, seg, t0=None, **planted):
        """A segment; with t0, its planted twin goes into the call: rows, col, node, device_graph, ref_graph, ptr (local
        device arc offsets: {state: value})."""
        rows, col, g, node = seg
        self.clean.add(rows, col, g, node, gap=1)
        if t0 is not None:
            self.at[len(self.call.T)] = t0
        for j, v in planted.get("ptr", {}).items():
            first = int(sum(len(x["arc_src"]) for x in self.call.graphs))
            self.call.device_ptr[len(self.call.col) + j] = first + v
        self.call.add(planted.get("rows", rows), planted.get("col", col), g, planted.get("node", node), gap=1)
        self.dev.append(planted.get("device_graph", g))
        self.refg.append(planted.get("ref_graph", self.dev[-1]))
        return self

    def done(self):
        if any(d is not g for d, g in zip(self.dev, self.call.graphs)):
            self.call.device_graphs = self.dev
        if any(r is not d for r, d in zip(self.refg, self.dev)):
            self.call.ref_graphs = self.refg
        return self

    def modes(self):
        """The launches (wave, workgroup) of each mode, from the state counts."""
        S = np.diff(api.pack_graphs(self.call.graphs)["statePtr"])
        return ((1, (int((S <= 256).any()), int((S > 256).any()))), (2, (0, 1)), (0, (int((S <= 64).any()), int((S > 64).any()))))


def row_plants():
    out = {}
    for group, shapes in GROUPS.items():
        for kind in ("nan column", "nan frame", "+inf frame", "-inf frame", "+inf meets -inf final"):
            p = Plant().add(segment(7, 9, 1))
            for i, (S, T, t0) in enumerate(shapes):
                rows, col, g, node = seg = segment(S, T, 10 * len(out) + i)
                bad, j = rows.copy(), heavy(seg, t0)
                if kind == "nan column":  # one state's column from t0 on: the skip arcs go round it
                    bad[t0:, col[j]] = np.nan
                elif kind == "+inf meets -inf final":  # the term of the total is a NaN at t0 and is skipped; the +inf then spreads
                    t0, j = min(t0, T - 2), min(j, len(col) - 3)  # (a frame and two states after it for the +inf to reach)
                    g = dict(g, final_lp=g["final_lp"].copy())
                    g["final_lp"][j] = -np.inf
                    seg = (rows, col, g, node)
                    bad[t0, col[j]] = np.inf
                else:
                    bad[t0, :] = dict((("nan frame", np.nan), ("+inf frame", np.inf), ("-inf frame", -np.inf)))[kind]
                p.add(seg, t0, rows=bad)
            out[f"{kind}, {group}"] = p.done()
        for handle, tag in ((FLOOR32, "f32"), (FLOOR16, "f16")):
            for kind in ("column", "frame"):  # the same plants as probabilities under a floor: one segment per value
                p = Plant(handle).add(segment(7, 9, 1, handle))
                for i, (S, T, t0) in enumerate(shapes):
                    for k, v in enumerate(AS_PROBS):
                        rows, col, g, node = seg = segment(S, T, 10 * len(out) + 4 * i + k, handle)
                        bad = rows.copy()
                        if kind == "column":
                            bad[t0:, col[heavy(seg, t0, handle)]] = v
                        else:
                            bad[t0, :] = v
                        p.add(seg, t0, rows=bad)
                out[f"{tag} probabilities 0, < 0, nan, +inf in a {kind}, {group}"] = p.done()
    return out


def index_plants():
    out = {}
    for group, shapes in GROUPS.items():
        for handle, tag in ((None, "scores"), (FLOOR32, "f32")):
            p = Plant(handle).add(segment(7, 9, 2, handle))
            for i, (S, T, _) in enumerate(shapes):
                rows, col, g, node = seg = segment(S, T, 3000 + 10 * len(out) + i, handle)
                j, ld = heavy(seg, 0, handle), rows.shape[1]
                for c in (ld, -1):  # the sibling's set: the row stride, -1
                    p.add(seg, 0, col=col[:j] + [c] + col[j + 1:])
                if handle is not None:
                    for nd in (WIDTH, -1):  # the handle's width, -1
                        p.add(seg, 0, node=node[:j] + [nd] + node[j + 1:])
            out[f"columns{' and nodes' if handle else ''} out of range, {tag}, {group}"] = p.done()
    # the DEVICE copy of the arc sources outside [0, S) while the host table is sound: a NaN candidate, nothing read
    for group, shapes in (("staged, k1", ((5, 9), (64, 9))), ("staged and unstaged, k4", ((130, 9), (ARCS, 9)))):
        p = Plant().add(segment(7, 9, 3))
        for i, (S, T) in enumerate(shapes):
            for k, bad in enumerate(BAD_SOURCES):
                rows, col, g, node = seg = segment(S, T, 4000 + 10 * i + k)
                n = len(col)
                src = np.array(g["arc_src"], np.int32)
                for j in (n // 2, n - 1):
                    src[int(g["arc_ptr"][j]) + 1] = n if bad is None else bad  # its second arc; the others remain
                p.add(seg, 1, device_graph=dict(g, arc_src=src))
        out[f"device arc sources out of range, {group}"] = p.done()
    # the DEVICE arc offsets: one below the segment's first arc, one above its last.  The kernels clamp every offset into
    # [0, the host table's arcs of the segment] (fdnn_fb_frames.hip: "inside the host table's count whatever the device copy
    # holds"), so no arc index leaves the segment's arcs: the restatement runs over clamped()
    p = Plant().add(segment(7, 9, 4))
    for i, (S, T) in enumerate(((9, 9), (64, 17), (65, 9), (300, 9))):
        rows, col, g, node = seg = segment(S, T, 5000 + i)
        n, arcs = len(col), len(g["arc_src"])
        ptr = np.array(g["arc_ptr"], np.int64)
        edits = {n // 3: -2 - i, 2 * n // 3: arcs + 4 + i}
        for j, v in edits.items():
            ptr[j] = v
        p.add(seg, 1, ptr=edits, ref_graph=clamped(g, ptr))
    out["device arc offsets below and above the segment"] = p.done()
    return out


CARRIES = ("one nan", "all nan", "one +inf", "all -inf", "-3e38 beside -1")


def carry_plants():
    out = {}
    # two calls a kind: in mode 1 a launch's states per lane are its largest segment's, so 65 (K = 2) and 130 (K = 4) are apart
    for kind, tag, sizes in ((k, t, s) for k in CARRIES for t, s in (("", (7, 5, 65, 300)), (", k4", (7, 130)))):
        p = Plant()
        rng = np.random.default_rng(77 + len(tag))
        clean_in, bad_in = [], []
        for i, S in enumerate(sizes):
            a = rng.uniform(-30, -5, S).astype(np.float32)
            b = a.copy()
            if i:
                if kind == "one nan":
                    b[np.argmax(a)] = np.nan  # (the value that carries most of the mass)
                elif kind == "all nan":
                    b[:] = np.nan
                elif kind == "one +inf":
                    b[np.argmax(a)] = np.inf
                elif kind == "all -inf":
                    b[:] = -np.inf
                else:
                    b[:] = -1.0
                    b[::2] = -3e38
            p.add(segment(S, 9, 6000 + i + 10 * len(tag)), 0 if i else None)
            clean_in.append(a), bad_in.append(b)
        p.alpha_in, p.clean_in = np.concatenate(bad_in), np.concatenate(clean_in)
        out[f"alpha_in: {kind}{tag}"] = p.done()
    return out


_plants = {}


def plants():
    if not _plants:
        for part in (row_plants(), index_plants(), carry_plants()):
            _plants.update(part)
    return _plants


PLANT_NAMES = tuple(f"{kind}, {group}" for group in GROUPS for kind in ("nan column", "nan frame", "+inf frame", "-inf frame", "+inf meets -inf final")) \
    + tuple(f"{tag} probabilities 0, < 0, nan, +inf in a {kind}, {group}" for group in GROUPS for tag in ("f32", "f16") for kind in ("column", "frame")) \
    + tuple(f"columns{' and nodes' if tag == 'f32' else ''} out of range, {tag}, {group}" for group in GROUPS for tag in ("scores", "f32")) \
    + ("device arc sources out of range, staged, k1", "device arc sources out of range, staged and unstaged, k4", "device arc offsets below and above the segment") \
    + tuple(f"alpha_in: {kind}{tag}" for kind in CARRIES for tag in ("", ", k4"))


def frames_of(c, seg):
    a = int(np.sum(c.T[:seg]))
    return slice(a, a + c.T[seg])


@pytest.mark.parametrize("name", PLANT_NAMES)
def test_planted_bad_input_in_every_form(name):
    """Anchored and free, modes 1, 2 and 0 with the launch counts, uncut and cut at T / 2 with the device's own carry row:
    frame_total the restatement's bytes, alpha_out under same_but_nan."""
    import torch

    assert set(plants()) == set(PLANT_NAMES)
    p = plants()[name]
    lp = LL.priors(WIDTH) if p.handle is not None else None
    anchored, free = held(torch, p.call, p.handle, lp, modes=p.modes(), alpha_in=p.alpha_in, equal=same_but_nan)
    assert not np.isnan(anchored).any() and not np.isnan(free).any()  # consequence (c)
    clean = frames_of(p.call, 0)
    assert np.isfinite(anchored[clean]).all() and np.isfinite(free[clean]).all()  # the clean segment beside them is untouched
    if name.startswith(("nan frame", "-inf frame")):  # -inf from the planted frame on; a free start recovers at the next frame
        for seg, t0 in p.at.items():
            a, f = anchored[frames_of(p.call, seg)], free[frames_of(p.call, seg)]
            assert np.isneginf(a[t0:]).all() and np.isneginf(f[t0]) and np.isfinite(f[t0 + 1:]).all() and np.isfinite(a[:t0]).all(), (seg, t0)
    if name.startswith("alpha_in: all -inf"):
        for seg in p.at:
            a, f = anchored[frames_of(p.call, seg)], free[frames_of(p.call, seg)]
            assert np.isneginf(a).all() and np.isfinite(f).all()


@pytest.mark.parametrize("free", (False, True), ids=("anchored", "free"))
@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("n_segs", (3, 65))
def test_the_carry_row_in_place(n_segs, mode, free):
    """d_alpha_out == d_alpha_in, ONE buffer (fdnn_fb_frames.hpp: allowed): a segment's sweep loads its carry row before it
    stores anything and touches no other segment's states, so the second half of a cut call gives the two-buffer run's
    bytes -- over 65 segments a second launch works on the same buffer."""
    import torch

    rng = np.random.default_rng(50 + n_segs)
    c = FramesCall()
    for i in range(n_segs):
        S = 300 if i == 1 else int(rng.integers(1, 65)) if n_segs > 3 else (5, 0, 130)[i]
        c.add(AC.scores(int(rng.integers(2, 20)), 11, 700 + i) * SCALE, rng.integers(0, 11, S).tolist(), open_chain(S, rng), gap=int(rng.integers(0, 4)))
    a, b = c.cut(False), c.cut(True)
    first = a.device(torch, mode=mode, free=free)
    two = b.device(torch, mode=mode, free=free, alpha_in=first[1])
    one = b.device(torch, mode=mode, free=free, alpha_in=first[1], in_place=True)
    launches = {(3, 1): (1, 1, 2), (3, 2): (0, 1, 1), (65, 1): (2, 1, 3), (65, 2): (0, 2, 2)}[n_segs, mode]  # (every 64 segments a launch per form)
    assert same(one, two) and one[2] == two[2] == launches, one[2]
    want = c.ref(free=free)
    joined = np.concatenate([x for pair in zip(split(first[0], a.T), split(one[0], b.T)) for x in pair])
    assert same((joined, one[1]), want) and np.isfinite(want[0]).all()
