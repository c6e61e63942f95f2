"""The alignment-graph kernels alone (fdnn_align_graph_rows_device) on planted device rows: path and total are the BYTES of the
host restatement (api.align_graph_ref, held to numpy and to brute force by tests/test_align_graph_host.py) in both forced
forms, at the lane-block edges of the wave form and on both sides of its limit, at the most states, with a handle of each type
and none, over 1 .. 65 segments, at the edges of the arc-staging and back-pointer caps, off-alignment row bases, with guard
words around path, total and scratch."""
import numpy as np
import pytest

import align_cases as AC
import align_graph_cases as GC
import loglik_cases as LL
from fast_dnn_amd import api

pytestmark = pytest.mark.gpu
GUARD = 4
WIDTH = 67  # nodes of the handles used here
HANDLES = (None, (-np.inf, api.LOGLIK_F32), (-20.0, api.LOGLIK_F16))
FILL = 0x5a5a5a5a


class Call:
    """One fdnn_align_graph_rows_device call's host side: segments of rows [T][ld], their graphs, columns (and nodes)."""

    def __init__(self):
        self.blocks, self.T, self.off, self.ld, self.col, self.node, self.graphs = [], [], [], [], [], [], []
        self.at = 0

    def add(self, rows, col, graph, node=None, gap=0):
        rows = np.ascontiguousarray(rows, np.float32)
        assert len(col) == len(graph["states"])
        self.at += gap
        self.blocks.append((self.at, rows))
        self.T.append(rows.shape[0]), self.off.append(self.at), self.ld.append(rows.shape[1])
        self.at += rows.size
        self.col.extend(col)
        self.node.extend(node if node is not None else [0] * len(col))
        self.graphs.append(graph)
        return self

    def flat(self):
        out = np.full(self.at, np.nan, np.float32)  # (gaps between blocks are never read)
        for at, rows in self.blocks:
            out[at:at + rows.size] = rows.ravel()
        return out

    def ref(self, handle=None, lp=None):
        kw = dict(stateNode=self.node, log_prior=lp, floor=handle[0], type=handle[1]) if handle is not None else {}
        return api.align_graph_ref(self.flat(), self.T, self.off, self.ld, api.pack_graphs(self.graphs), self.col, **kw)

    def device(self, torch, handle=None, lp=None, mode=0, shift=0):
        """-> (path, total, launches) of the call under kernel mode `mode`, the rows' base `shift` floats off its allocation."""
        api.set_align_graph_kernel(mode)
        try:
            ll = api.Loglik(lp, *handle) if handle is not None else None
            flat, g = self.flat(), api.pack_graphs(self.graphs)
            d_rows = torch.zeros(flat.size + 4, dtype=torch.float32, device="cuda")
            d_rows[shift:shift + flat.size] = torch.from_numpy(flat).cuda()
            dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).cuda()
            ptr = lambda d: d.data_ptr() if d is not None and d.numel() else 0
            d_col, d_node = dev(self.col, np.int32), dev(self.node, np.int32)
            d_ap, d_src, d_lp = dev(g["arcPtr"], np.int32), dev(g["arcSrc"], np.int32), dev(g["arcLp"], np.float32)
            d_start = dev(g["startLp"], np.float32) if g["startLp"] is not None else None
            d_final = dev(g["finalLp"], np.float32) if g["finalLp"] is not None else None
            words = api.align_graph_scratch_words(self.T, g["statePtr"])
            d_scr = torch.full((words + 2 * GUARD,), FILL, dtype=torch.int32, device="cuda")
            rows, n = int(np.sum(self.T)), len(self.T)
            d_path = torch.full((rows + 2 * GUARD,), -7, dtype=torch.int32, device="cuda")
            d_total = torch.full((n + 2 * GUARD,), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            before = api.align_graph_launches()
            api.align_graph_rows_device(ll, d_rows.data_ptr() + 4 * shift, self.T, self.off, self.ld, g["statePtr"], g["arcPtr"], d_col.data_ptr(),
                                        d_node.data_ptr() if ll else 0, d_ap.data_ptr(), ptr(d_src), ptr(d_lp), ptr(d_start), ptr(d_final),
                                        d_scr.data_ptr() + 4 * GUARD if words else 0, words, d_path.data_ptr() + 4 * GUARD, d_total.data_ptr() + 4 * GUARD)
            torch.cuda.synchronize()
            after = api.align_graph_launches()
            p, t = d_path.cpu().numpy(), d_total.cpu().numpy()
            s = torch.cat([d_scr[:GUARD], d_scr[GUARD + words:]]).cpu().numpy()  # (the guard words alone: the scratch may be large)
            assert (p[:GUARD] == -7).all() and (p[GUARD + rows:] == -7).all() and (t[:GUARD] == -7).all() and (t[GUARD + n:] == -7).all()
            assert s.size == 2 * GUARD and (s == FILL).all()
            if ll:
                ll.delete()
            return p[GUARD:GUARD + rows], t[GUARD:GUARD + n], tuple(b - a for a, b in zip(before, after))
        finally:
            api.set_align_graph_kernel(0)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def skip_chain(S, rng):
    """State j from j, j - 1 and j - 2 (in-degree 3), arc scores ln U: a finite path wherever T >= S / 2, whatever the rows."""
    ptr, src = [0], []
    for j in range(S):
        src.extend([s for s in (j, j - 1, j - 2) if s >= 0])
        ptr.append(len(src))
    return dict(states=np.zeros(S, np.int32), arc_ptr=np.array(ptr, np.int32), arc_src=np.array(src, np.int32),
                arc_lp=np.log(rng.uniform(0.05, 0.95, len(src))).astype(np.float32), start_lp=None, final_lp=None)


WAVE_STATES = 256  # the wave form's most states where it is forced; the rule takes it up to 64 (asserted against the library's limits below)


def both_forms(torch, c, handle=None, lp=None, wave_launches=(1, 0)):
    """The call in every kernel mode against the restatement -> the restatement's (path, total).  wave_launches: the launches
    per form where the wave form is forced wherever it is allowed."""
    want = c.ref(handle, lp)
    wave = c.device(torch, handle, lp, mode=1)
    wg = c.device(torch, handle, lp, mode=2)
    assert same(wave[:2], want) and wave[2] == wave_launches, wave[2]
    assert same(wg[:2], want) and wg[2] == (0, 1), wg[2]
    rule = c.device(torch, handle, lp, mode=0)
    S = np.diff(api.pack_graphs(c.graphs)["statePtr"])
    assert same(rule[:2], want) and rule[2] == (int((S <= 64).any()), int((S > 64).any())), rule[2]
    return want


def shaped_call(S, handle, seed, ld=37, Ts=None):
    """T = 1, 2 on random graphs (in-degrees 0 .. 3, backward arcs, several start and final states), T = S + 1 on a skip chain
    and on a random graph; columns (and nodes) repeat."""
    rng = np.random.default_rng(seed)
    c = Call()
    Ts = Ts or (1, 2, S + 1, S + 1)
    for i, T in enumerate(Ts):
        rows = AC.probs(T, ld, seed + i) if handle is not None else AC.scores(T, ld, seed + i)
        g = skip_chain(S, rng) if i == 2 else GC.random_graph(S, rng, starts=max(3, S // 4), finals=max(3, S // 4))
        c.add(rows, rng.integers(0, ld, S).tolist(), g, rng.integers(0, WIDTH, S).tolist(), gap=i)
    return c


@pytest.mark.parametrize("handle", HANDLES, ids=("scores", "f32", "f16"))
@pytest.mark.parametrize("S", (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025))
def test_shapes_in_both_forms(S, handle):
    """The lane-block edges of the wave form (1, 2 and 4 states a lane), both sides of its limit, and the chain form's limit."""
    import torch

    assert api.align_graph_limits()["wave_states"] == WAVE_STATES and api.align_graph_limits()["wave_rule_states"] == 64
    lp = LL.priors(WIDTH)
    c = shaped_call(S, handle, 100 + S)
    want = both_forms(torch, c, handle, lp, wave_launches=(1, 0) if S <= WAVE_STATES else (0, 1))
    T = np.cumsum([0] + c.T)
    assert np.isfinite(want[1][2]) and (want[0][T[2]:T[3]] >= 0).all()  # the skip chain always has a path
    assert np.isfinite(want[1]).sum() >= 2


def test_the_most_states():
    """S = 16384 over 8-column rows at T = 1, 2 and S + 1, workgroup form, scores: 16385 frames of 8192 back-pointer words each,
    537 MB of scratch, half the cap of a call.  The graph is a skip chain (state j from j, j - 1, j - 2) that starts and ends
    in one state in twenty, so the short segments have paths too; state S - 1 also takes a long skip from state 17."""
    import torch

    S = api.align_graph_limits()["max_states"]
    rng = np.random.default_rng(5)
    c = Call()
    for i, T in enumerate((1, 2, S + 1)):
        g = skip_chain(S, rng)
        g["start_lp"] = np.where(rng.random(S) < 0.05, 0.0, -np.inf).astype(np.float32)
        g["final_lp"] = np.where(rng.random(S) < 0.05, 0.0, -np.inf).astype(np.float32)
        if i == 2:
            g["arc_src"][-1] = 17  # a long skip: state S - 1 from state 17
        c.add(AC.scores(T, 8, 6 + i), rng.integers(0, 8, S).tolist(), g)
    words = api.align_graph_scratch_words(c.T, api.pack_graphs(c.graphs)["statePtr"])
    assert words == (1 + 2 + S + 1) * S // 2 and 4 * words > (api.align_graph_limits()["scratch_cap_mib"] << 20) // 2
    want = c.ref()
    assert np.isfinite(want[1]).all() and (want[0] >= 0).all()
    got = c.device(torch)
    assert same(got[:2], want) and got[2] == (0, 1)


def test_in_degrees_and_a_state_with_300_arcs():
    import torch

    rng = np.random.default_rng(11)
    S = 90
    g = GC.random_graph(S, rng, starts=4, finals=4)
    deg = np.diff(g["arc_ptr"])
    assert set(deg.tolist()) == {0, 1, 2, 3}
    # state 40 gets 300 arcs, every state as a source several times over
    at = int(g["arc_ptr"][40])
    many = rng.integers(0, S, 300).astype(np.int32)
    g["arc_src"] = np.concatenate([g["arc_src"][:at], many, g["arc_src"][int(g["arc_ptr"][41]):]])
    g["arc_lp"] = np.concatenate([g["arc_lp"][:at], np.log(rng.uniform(0.05, 0.95, 300)).astype(np.float32), g["arc_lp"][int(g["arc_ptr"][41]):]])
    g["arc_ptr"] = np.concatenate([g["arc_ptr"][:41], g["arc_ptr"][41:] + 300 - deg[40]]).astype(np.int32)
    g["final_lp"][40] = 0.0
    c = Call().add(AC.scores(70, 19, 12), rng.integers(0, 19, S).tolist(), g).add(AC.scores(5, 19, 13), rng.integers(0, 19, S).tolist(), g)
    want = both_forms(torch, c)
    assert np.isfinite(want[1]).all()


@pytest.mark.parametrize("arcs", (4095, 4096, 4097))
def test_the_arc_staging_cap_at_its_edge(arcs):
    """A segment with one arc fewer than the wave form stages in LDS, exactly as many, and one more (read from the L2 every
    frame), beside a small staged segment in the same launch."""
    import torch

    assert api.align_graph_limits()["lds_arcs"] == 4096
    rng = np.random.default_rng(arcs)
    S = 256
    deg = np.full(S, 16)
    deg[0] += arcs - 16 * S  # one arc fewer, as many, one more
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    assert ptr[-1] == arcs
    src = rng.integers(0, S, arcs).astype(np.int32)
    src[ptr[:-1]] = np.arange(S)  # a self-loop first
    g = dict(states=np.zeros(S, np.int32), arc_ptr=ptr, arc_src=src, arc_lp=np.log(rng.uniform(0.05, 0.95, arcs)).astype(np.float32),
             start_lp=np.zeros(S, np.float32), final_lp=np.zeros(S, np.float32))
    c = Call().add(AC.scores(12, 23, 1), rng.integers(0, 23, S).tolist(), g).add(AC.scores(9, 23, 2), rng.integers(0, 23, 5).tolist(), skip_chain(5, rng))
    want = both_forms(torch, c)
    assert np.isfinite(want[1]).all()


def test_back_pointers_at_the_lds_cap():
    """4095, 4096 and 4097 back-pointer words: the first two stay in LDS, the third goes through the scratch."""
    import torch

    assert api.align_graph_limits()["lds_bp_words"] == 4096
    rng = np.random.default_rng(21)
    for (T, S), words in (((130, 63), 0), ((128, 64), 0), ((4097, 2), 4097)):
        c = Call().add(AC.scores(T, 7, T), rng.integers(0, 7, S).tolist(), skip_chain(S, rng))
        assert api.align_graph_scratch_words(c.T, [0, S]) == words
        want = both_forms(torch, c)
        assert np.isfinite(want[1]).all()
    c = shaped_call(70, None, 22, ld=13, Ts=(90, 3000, 20))  # LDS, scratch and LDS in one launch
    assert api.align_graph_scratch_words(c.T, [0, 70, 140, 210]) == 3000 * 35
    both_forms(torch, c)


def test_graph_shapes():
    import torch

    ninf = -np.inf
    rows = AC.scores(9, 4, 31)
    f32 = lambda *v: np.array(v, np.float32)
    i32 = lambda *v: np.array(v, np.int32)
    # a two-state loop 0 <-> 1 without self-loops, entered in either: the path alternates
    loop = dict(states=i32(0, 0), arc_ptr=i32(0, 1, 2), arc_src=i32(1, 0), arc_lp=f32(-0.5, -0.25), start_lp=f32(0, 0), final_lp=f32(0, 0))
    # backward arcs: 2 -> 0, 3 -> 1 beside the chain
    back = dict(states=i32(0, 0, 0, 0), arc_ptr=i32(0, 2, 5, 7, 9), arc_src=i32(0, 2, 1, 0, 3, 2, 1, 3, 2), arc_lp=f32(-1, -.1, -1, -.2, -.1, -1, -.3, -1, -.1),
                start_lp=None, final_lp=None)
    # several start and final states with different values
    ends = dict(back, start_lp=f32(-2, -0.5, ninf, -1), final_lp=f32(ninf, -1, -0.5, -3))
    # a final state that cannot be reached: state 3 has no arcs and is no start state
    lost = dict(states=i32(0, 0, 0, 0), arc_ptr=i32(0, 1, 3, 5, 5), arc_src=i32(0, 1, 0, 2, 1), arc_lp=f32(0, 0, 0, 0, 0), start_lp=None, final_lp=None)
    # a state without arcs that is a start state: reachable at t = 0 only
    once = dict(states=i32(0, 0), arc_ptr=i32(0, 0, 2), arc_src=i32(1, 0), arc_lp=f32(-1, -1), start_lp=None, final_lp=None)
    c = Call()
    for g in (loop, back, ends, lost, once):
        c.add(rows[:, :len(g["states"])] if len(g["states"]) < 4 else rows, list(range(len(g["states"]))), g)
    want = both_forms(torch, c)
    T = 9
    assert set(np.abs(np.diff(want[0][:T])).tolist()) == {1} and np.isfinite(want[1][:3]).all()
    assert (np.diff(want[0][T:2 * T]) < 0).any() or (np.diff(want[0][2 * T:3 * T]) < 0).any()  # a backward arc is on a best path
    assert np.isneginf(want[1][3]) and (want[0][3 * T:4 * T] == -1).all()
    assert np.isfinite(want[1][4]) and want[0][4 * T:].tolist() == [0] + [1] * 8


def test_planted_ties_and_the_arc_order():
    import torch

    c, r = Call(), Call()
    for seed in range(3):
        rows, g, col = GC.silence_case(seed, integers=True)
        c.add(rows, col.tolist(), g)
        r.add(rows, col.tolist(), GC.reversed_arcs(g))
    ints = np.random.default_rng(8).integers(-3, 4, (40, 9)).astype(np.float32)
    rg = GC.random_graph(30, np.random.default_rng(18), integers=True, starts=5, finals=5)  # (a seed with a path: 15 % of the frames change)
    cols = np.random.default_rng(10).integers(0, 9, 30).tolist()
    c.add(ints, cols, rg), r.add(ints, cols, GC.reversed_arcs(rg))
    c.add(np.zeros((12, 5), np.float32), list(range(5)), api.chain_graph(list(range(5))))  # all-zero scores: 0, 1, .., S - 1, S - 1, ..
    r.add(np.zeros((12, 5), np.float32), list(range(5)), GC.reversed_arcs(api.chain_graph(list(range(5)))))  # the move first: as late as possible
    a, b = both_forms(torch, c), both_forms(torch, r)
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.isfinite(a[1]).all()
    for s in range(3):
        assert not np.array_equal(a[0][129 * s:129 * (s + 1)], b[0][129 * s:129 * (s + 1)])
    assert a[0][-12:].tolist() == [0, 1, 2, 3, 4] + [4] * 7 and b[0][-12:].tolist() == [0] * 8 + [1, 2, 3, 4]


def test_sources_columns_and_nodes_out_of_range():
    import torch

    lp = LL.priors(WIDTH)
    rng = np.random.default_rng(40)
    chain4 = api.chain_graph([0, 0, 0, 0])
    wide = skip_chain(6, rng)
    c = Call()
    c.add(AC.scores(9, 4, 13), [0, 1, 2, 4], chain4)    # the last state's column at the row stride: no path, -inf, never a NaN
    c.add(AC.scores(9, 4, 14), [0, -1, 2, 3], chain4)   # nothing leaves a NaN
    c.add(AC.scores(9, 6, 15), [0, 1, 7, 3, 4, 5], wide)  # ... but the skip goes round it
    for bad in (4, -1, 1 << 16, -(1 << 31), 65535):     # a source outside [0, S): that candidate is a NaN, nothing is read
        c.add(AC.scores(9, 4, 16), [0, 1, 2, 3], dict(chain4, arc_src=np.array([0, 1, bad, 2, 1, 3, 2], np.int32)))
    skip_bad = dict(wide, arc_src=wide["arc_src"].copy())
    skip_bad["arc_src"][int(wide["arc_ptr"][3]) + 1] = 99  # state 3's arc from state 2; the others remain
    c.add(AC.scores(9, 6, 17), list(range(6)), skip_bad)
    want = both_forms(torch, c)
    assert np.isneginf(want[1][:2]).all() and np.isfinite(want[1][2]) and 2 not in want[0][18:27]
    assert np.isneginf(want[1][3:8]).all() and np.isfinite(want[1][8]) and (want[0][:18] == -1).all()
    # a node outside the handle's width: a NaN emission, nothing read
    d = Call()
    for i, nodes in enumerate(([1, 2, 3, WIDTH], [1, -1, 5, 3], [1, 2, 3, 4])):
        d.add(AC.probs(9, 5, 15 + i), [0, 1, 2, 3], chain4, nodes)
    handle = (-20.0, api.LOGLIK_F32)
    want = both_forms(torch, d, handle, lp)
    assert np.isneginf(want[1][:2]).all() and np.isfinite(want[1][2]) and (want[0][:18] == -1).all()


@pytest.mark.parametrize("n_segs,launches", ((1, 1), (2, 1), (64, 1), (65, 2)))
def test_segments_per_launch(n_segs, launches):
    """Segments of unequal T and S, all inside the rule's wave form; 65 need a second launch.  With graphs on both sides of
    the rule's limit every 64 segments go as one launch per form."""
    import torch

    rng = np.random.default_rng(20 + n_segs)
    c = Call()
    for i in range(n_segs):
        S = int(rng.integers(1, 65))
        T = S // 2 + int(rng.integers(1, 40))
        c.add(AC.scores(T, 11, 400 + i), rng.integers(0, 11, S).tolist(), skip_chain(S, rng) if i % 2 else GC.random_graph(S, rng), gap=int(rng.integers(0, 4)))
    want = c.ref()
    got = c.device(torch)
    assert same(got[:2], want) and got[2] == (launches, 0) and np.isfinite(want[1]).sum() >= n_segs // 2
    if n_segs == 2:
        c.add(AC.scores(600, 11, 600), rng.integers(0, 11, 1030).tolist(), skip_chain(1030, rng))
        got = c.device(torch)
        assert same(got[:2], c.ref()) and got[2] == (1, 1)


def test_a_5_state_and_a_1000_state_segment_in_one_launch():
    """The rows of d, the states per lane and the staged arcs are the LAUNCH's largest: a 5-state segment beside a 250-state
    one in the wave form and beside 1000-state ones in the workgroup form (one launch of each where the wave form is allowed,
    ONE launch where it is not), its back-pointers in LDS while the long ones' go through the scratch; both handles."""
    import torch

    lp = LL.priors(WIDTH)
    for handle in (None, (-20.0, api.LOGLIK_F16)):
        rng = np.random.default_rng(900)
        c = Call()
        for i, (T, S) in enumerate(((20, 5), (600, 1000), (9, 9), (1001, 1000), (300, 250))):
            rows = AC.probs(T, 23, 910 + i) if handle is not None else AC.scores(T, 23, 910 + i)
            c.add(rows, rng.integers(0, 23, S).tolist(), skip_chain(S, rng), rng.integers(0, WIDTH, S).tolist(), gap=i)
        assert api.align_graph_scratch_words(c.T, [0, 5, 1005, 1014, 2014, 2264]) == (600 + 1001) * 500 + 300 * 125
        want = both_forms(torch, c, handle, lp, wave_launches=(1, 1))
        assert np.isfinite(want[1]).all() and (want[0] >= 0).all()


@pytest.mark.parametrize("shift", (1, 2, 3))
def test_row_bases_off_16_bytes(shift):
    import torch

    lp = LL.priors(WIDTH)
    for handle in (None, (-np.inf, api.LOGLIK_F32)):
        c = shaped_call(70, handle, 700 + shift, ld=13, Ts=(90, 50, 117, 3))
        want = c.ref(handle, lp)
        for mode in (1, 2):
            assert same(c.device(torch, handle, lp, mode=mode, shift=shift)[:2], want), (handle, mode)


def test_the_chain_graph_gives_the_chain_kernels_bytes():
    """On NaN-free inputs the chain as a graph returns api.align_rows_device's path and total byte for byte, T < S included."""
    import torch

    lp = LL.priors(WIDTH)
    for handle in HANDLES:
        rng = np.random.default_rng(55)
        c, chain = Call(), []
        for i, (T, S) in enumerate(((40, 12), (130, 40), (3, 5), (1, 1), (300, 257), (1100, 1030))):
            rows = AC.probs(T, 29, 60 + i) if handle is not None else AC.scores(T, 29, 60 + i)
            sl, nl = AC.transitions(S, 70 + i)
            c.add(rows, rng.integers(0, 29, S).tolist(), api.chain_graph(np.zeros(S, np.int32), sl, nl), rng.integers(0, WIDTH, S).tolist(), gap=i)
            chain.append((sl, nl))
        got = c.device(torch, handle, lp)
        assert same(got[:2], c.ref(handle, lp)) and got[2] == (1, 1)
        # the same rows through the chain kernels
        ll = api.Loglik(lp, *handle) if handle is not None else None
        sp = np.concatenate([[0], np.cumsum([len(g["states"]) for g in c.graphs])]).astype(np.int32)
        dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).cuda()
        d_rows, d_col, d_node = dev(np.nan_to_num(c.flat()), np.float32), dev(c.col, np.int32), dev(c.node, np.int32)
        d_sl, d_nl = dev(np.concatenate([s for s, _ in chain]), np.float32), dev(np.concatenate([n for _, n in chain]), np.float32)
        words = api.align_scratch_words(c.T, sp)
        d_scr = torch.zeros(max(words, 2), dtype=torch.int32, device="cuda")
        d_path = torch.zeros(int(np.sum(c.T)), dtype=torch.int32, device="cuda")
        d_total = torch.zeros(len(c.T), dtype=torch.float32, device="cuda")
        api.align_rows_device(ll, d_rows.data_ptr(), c.T, c.off, c.ld, sp, d_col.data_ptr(), d_node.data_ptr() if ll else 0, d_sl.data_ptr(), d_nl.data_ptr(),
                              d_scr.data_ptr(), words, d_path.data_ptr(), d_total.data_ptr())
        torch.cuda.synchronize()
        if ll:
            ll.delete()
        assert same((d_path.cpu().numpy(), d_total.cpu().numpy()), got[:2]), handle
        assert np.isneginf(got[1][2]) and np.isfinite(np.delete(got[1], 2)).all()


def test_argument_errors_launch_nothing():
    import torch

    before = api.align_graph_launches()
    L, i32, i64 = api.lib(), api.C.POINTER(api.C.c_int), api.C.POINTER(api.C.c_longlong)
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()

    def call(T=(9,), off=(0,), ld=(37,), sp=(0, 5), ap=(0, 1, 2, 3, 4, 5), rows=p, col=p, d_ap=p, d_src=p, d_lp=p, path=p, total=p, scratch=0, words=0):
        a = [np.array(v, t) for v, t in ((T, np.int32), (off, np.int64), (ld, np.int32), (sp, np.int32))]
        h_ap = None if ap is None else np.array(ap, np.int32).ctypes.data_as(i32)
        return L.fdnn_align_graph_rows_device(None, rows, a[0].ctypes.data_as(i32), a[1].ctypes.data_as(i64), a[2].ctypes.data_as(i32),
                                              a[3].ctypes.data_as(i32), h_ap, 1, col, None, d_ap, d_src, d_lp, None, None, scratch, words, path, total, None)

    too_many = tuple(np.arange(6) * 40000)  # 200 000 arcs over 5 states
    for bad in (dict(T=(0,)), dict(ld=(0,)), dict(off=(-1,)), dict(sp=(0, 0)), dict(sp=(1, 6)), dict(sp=(0, 16385)), dict(rows=None), dict(col=None),
                dict(path=None), dict(total=None), dict(rows=p + 2), dict(scratch=p + 2, words=9), dict(T=(3000,)),  # (3000 frames need scratch words: none given)
                dict(ap=None), dict(ap=(1, 1, 2, 3, 4, 5)), dict(ap=(0, 2, 1, 3, 4, 5)), dict(ap=too_many), dict(d_ap=None), dict(d_src=None), dict(d_lp=None)):
        assert call(**bad) == api.FDNN_E_ARG, bad
    with pytest.raises(api.FdnnError):
        api.set_align_graph_kernel(3)
    torch.cuda.synchronize()
    assert api.align_graph_launches() == before
