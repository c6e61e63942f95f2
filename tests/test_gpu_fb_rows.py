"""The forward-backward kernels alone (fdnn_fb_rows_device) on planted device rows: total and gamma are the BYTES of the host
restatement (api.fb_ref, held to float64 and to brute force by tests/test_fb_host.py) in both forced forms and under the rule,
at the lane-block edges of the wave form and on both sides of its limit and of the total's 256 partials, at the most states,
with a handle of each type and none, with gamma wanted and forward only, over 1 .. 65 segments, at the edge of the arc-staging
cap, off-alignment row bases, with guard words around gamma, total and scratch."""
import numpy as np
import pytest

import align_cases as AC
import align_graph_cases as GC
import fb_cases as FC
import loglik_cases as LL
from fast_dnn_amd import api

pytestmark = pytest.mark.gpu
GUARD = 4
WIDTH = 67  # nodes of the handles used here
HANDLES = (None, (-np.inf, api.LOGLIK_F32), (-20.0, api.LOGLIK_F16))
SCALE = np.float32(0.2)  # scores 0.2 (3 N(0, 1) - 5): many paths share the mass, so the occupancies are soft


class Call:
    """One fdnn_fb_rows_device call's host side: segments of rows [T][ld], their graphs, columns (and nodes)."""

    def __init__(self):
        self.blocks, self.T, self.off, self.ld, self.col, self.node, self.graphs = [], [], [], [], [], [], []
        self.at = 0
        self.transposed = None  # (a test may plant its own transposed tables)
        self.device_graphs = None  # (.. or device copies that differ from the host tables)

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

    def tables(self):
        g = api.pack_graphs(self.device_graphs or self.graphs)
        host = api.pack_graphs(self.graphs)
        return g, host, (self.transposed or api.fb_transpose(host))

    def ref(self, handle=None, lp=None, want_gamma=True):
        kw = dict(stateNode=self.node, log_prior=lp, floor=handle[0], type=handle[1]) if handle is not None else {}
        g, _, t = self.tables()
        return api.fb_ref(self.flat(), self.T, self.off, self.ld, g, self.col, want_gamma=want_gamma, transposed=t, **kw)

    def device(self, torch, handle=None, lp=None, mode=0, shift=0, want_gamma=True):
        """-> (total, gamma or None, launches) of the call under kernel mode `mode`, the rows' base `shift` floats off its allocation."""
        api.set_fb_kernel(mode)
        try:
            ll = api.Loglik(lp, *handle) if handle is not None else None
            flat = self.flat()
            g, host, t = self.tables()
            d_rows = torch.zeros(flat.size + 4, dtype=torch.float32, device="cuda")
            d_rows[shift:shift + flat.size] = torch.from_numpy(flat).cuda()
            dev = lambda a, ty: torch.from_numpy(np.ascontiguousarray(a, ty)).cuda()
            ptr = lambda d: d.data_ptr() if d is not None and d.numel() else 0
            d_col, d_node = dev(self.col, np.int32), dev(self.node, np.int32)
            d_ap, d_src, d_lp = dev(g["arcPtr"], np.int32), dev(g["arcSrc"], np.int32), dev(g["arcLp"], np.float32)
            d_tp, d_ts, d_tl = dev(t["tPtr"], np.int32), dev(t["tSrc"], np.int32), dev(t["tLp"], np.float32)
            d_start = dev(g["startLp"], np.float32) if g["startLp"] is not None else None
            d_final = dev(g["finalLp"], np.float32) if g["finalLp"] is not None else None
            words = api.fb_scratch_words(self.T, host["statePtr"], want_gamma)
            cells, n = int((np.asarray(self.T, np.int64) * np.diff(host["statePtr"])).sum()), len(self.T)
            assert words == (cells if want_gamma else 0)
            d_scr = torch.full((words + 2 * GUARD,), -9.0, dtype=torch.float32, device="cuda")
            d_gamma = torch.full((cells + 2 * GUARD,), -7.0, dtype=torch.float32, device="cuda")
            d_total = torch.full((n + 2 * GUARD,), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            before = api.fb_launches()
            api.fb_rows_device(ll, d_rows.data_ptr() + 4 * shift, self.T, self.off, self.ld, host["statePtr"], host["arcPtr"],
                               t["tPtr"] if want_gamma else None, d_col.data_ptr(), d_node.data_ptr() if ll else 0, d_ap.data_ptr(), ptr(d_src), ptr(d_lp),
                               ptr(d_start), ptr(d_final), d_tp.data_ptr() if want_gamma else 0, ptr(d_ts) if want_gamma else 0,
                               ptr(d_tl) if want_gamma else 0, d_scr.data_ptr() + 4 * GUARD if words else 0, words, d_total.data_ptr() + 4 * GUARD,
                               d_gamma.data_ptr() + 4 * GUARD if want_gamma else 0)
            torch.cuda.synchronize()
            after = api.fb_launches()
            gm, tt = d_gamma.cpu().numpy(), d_total.cpu().numpy()
            s = torch.cat([d_scr[:GUARD], d_scr[GUARD + words:]]).cpu().numpy()  # (the guard words alone: the scratch may be large)
            assert (gm[:GUARD] == -7).all() and (gm[GUARD + cells:] == -7).all() and (tt[:GUARD] == -7).all() and (tt[GUARD + n:] == -7).all()
            assert s.size == 2 * GUARD and (s == -9).all()
            if not want_gamma:
                assert (gm == -7).all()
            if ll:
                ll.delete()
            return tt[GUARD:GUARD + n], gm[GUARD:GUARD + cells] if want_gamma else None, tuple(b - a for a, b in zip(before, after))
        finally:
            api.set_fb_kernel(0)


def same(got, want):
    ok = np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    if want[1] is None:
        return ok and got[1] is None
    return ok and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def skip_chain(S, rng):
    """State j from j, j - 1 and j - 2 (in-degree 3), arc scores ln U: a finite path wherever T >= S / 2, whatever the rows."""
    ptr, src = [0], []
    for j in range(S):
        src.extend([s for s in (j, j - 1, j - 2) if s >= 0])
        ptr.append(len(src))
    return dict(states=np.zeros(S, np.int32), arc_ptr=np.array(ptr, np.int32), arc_src=np.array(src, np.int32),
                arc_lp=np.log(rng.uniform(0.05, 0.95, len(src))).astype(np.float32), start_lp=None, final_lp=None)


WAVE_STATES, RULE_STATES = 256, 64  # (asserted against the library's limits below)


def all_forms(torch, c, handle=None, lp=None, wave_launches=(1, 0)):
    """The call in every kernel mode, gamma wanted and forward only, against the restatement -> the restatement's (total,
    gamma).  wave_launches: the launches per form and direction where the wave form is forced wherever it is allowed."""
    want = c.ref(handle, lp)
    fwd = c.ref(handle, lp, want_gamma=False)
    assert fwd[1] is None and np.array_equal(fwd[0].view(np.uint32), want[0].view(np.uint32))
    S = np.diff(api.pack_graphs(c.graphs)["statePtr"])
    rule = (int((S <= RULE_STATES).any()), int((S > RULE_STATES).any()))
    for mode, per in ((1, wave_launches), (2, (0, 1)), (0, rule)):
        got = c.device(torch, handle, lp, mode=mode)
        assert same(got[:2], want), (mode, np.nonzero(got[0].view(np.uint32) != want[0].view(np.uint32))[0][:5],
                                     np.nonzero(got[1].view(np.uint32) != want[1].view(np.uint32))[0][:5])
        assert got[2] == per + per, (mode, got[2])
        got = c.device(torch, handle, lp, mode=mode, want_gamma=False)  # forward only: no backward launch, no scratch, gamma untouched
        assert same(got[:2], fwd) and got[2] == per + (0, 0), (mode, got[2])
    return want


def shaped_call(S, handle, seed, ld=37, Ts=None):
    """T = 1, 2 on random graphs (in-degrees 0 .. 3, backward arcs, several start and final states), T = S + 1 on a skip chain
    and on a random graph; columns (and nodes) repeat."""
    rng = np.random.default_rng(seed)
    c = Call()
    Ts = Ts or (1, 2, S + 1, S + 1)
    for i, T in enumerate(Ts):
        rows = AC.probs(T, ld, seed + i) if handle is not None else AC.scores(T, ld, seed + i) * SCALE
        g = skip_chain(S, rng) if i == 2 else GC.random_graph(S, rng, starts=max(3, S // 4), finals=max(3, S // 4))
        c.add(rows, rng.integers(0, ld, S).tolist(), g, rng.integers(0, WIDTH, S).tolist(), gap=i)
    return c


@pytest.mark.parametrize("handle", HANDLES, ids=("scores", "f32", "f16"))
@pytest.mark.parametrize("S", (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025))
def test_shapes_in_every_form(S, handle):
    """The lane-block edges of the wave form (1, 2 and 4 states a lane), both sides of its limit, and both sides of one and two
    states per partial of the total."""
    import torch

    lim = api.fb_limits()
    assert lim["wave_states"] == WAVE_STATES and lim["wave_rule_states"] == RULE_STATES and lim["partials"] == 256
    lp = LL.priors(WIDTH)
    c = shaped_call(S, handle, 100 + S)
    want = all_forms(torch, c, handle, lp, wave_launches=(1, 0) if S <= WAVE_STATES else (0, 1))
    assert np.isfinite(want[0][2]) and np.isfinite(want[0]).sum() >= 2 and not np.isnan(want[0]).any()  # the skip chain always has a path
    blocks = api.fb_gamma_blocks(want[1], c.T, api.pack_graphs(c.graphs)["statePtr"])
    at = 0
    for s, b in enumerate(blocks):
        col, node, rows = c.col[at:at + S], c.node[at:at + S], c.blocks[s][1]
        at += S
        if not np.isfinite(want[0][s]):
            assert (b.view(np.uint32) == 0).all()
            continue
        # the bytes are the restatement's; the restatement against float64 under the derived bound, M and A the case's own
        e = rows[:, col] if handle is None else api.loglik_entries_ref(np.tile(node, c.T[s]), rows[:, col].ravel(), lp, *handle).astype(np.float32).reshape(c.T[s], S)
        te, tb, ge, gb = FC.held(want[0][s], b, e, c.graphs[s])
        assert te <= tb and ge <= gb, (s, te, tb, ge, gb)
        assert (np.abs(b.sum(axis=1, dtype=np.float64) - 1) <= gb + S * 1.2e-38).all(), (s, gb)  # every row sums to 1
    if handle is None and S >= 63:  # not blind: the occupancies of the long skip-chain segment are soft
        assert (blocks[2].max(axis=1) < 0.9).mean() > 0.3


def test_the_most_states():
    """S = 16384 at T = 2, workgroup form, scores: 64 states a partial of the total, every state a final state."""
    import torch

    S = api.fb_limits()["max_states"]
    rng = np.random.default_rng(5)
    g = skip_chain(S, rng)
    g["start_lp"] = np.where(rng.random(S) < 0.5, 0.0, -np.inf).astype(np.float32)
    g["final_lp"] = np.log(rng.uniform(0.05, 0.95, S)).astype(np.float32)
    g["arc_src"][-1] = 17  # a long skip: state S - 1 from state 17
    c = Call().add(AC.scores(2, 8, 6) * SCALE, rng.integers(0, 8, S).tolist(), g)
    want = c.ref()
    assert np.isfinite(want[0]).all() and want[1].max() < 0.05
    for want_gamma in (True, False):
        got = c.device(torch, want_gamma=want_gamma)
        assert same(got[:2], c.ref(want_gamma=want_gamma)) and got[2] == (0, 1, 0, 1 if want_gamma else 0)


def test_in_degrees_and_a_state_with_300_arcs():
    import torch

    rng = np.random.default_rng(11)
    S = 90
    g = GC.random_graph(S, rng, starts=4, finals=4)
    deg = np.diff(g["arc_ptr"])
    assert set(deg.tolist()) == {0, 1, 2, 3}
    at = int(g["arc_ptr"][40])  # state 40 gets 300 arcs, every state as a source several times over
    many = rng.integers(0, S, 300).astype(np.int32)
    g["arc_src"] = np.concatenate([g["arc_src"][:at], many, g["arc_src"][int(g["arc_ptr"][41]):]])
    g["arc_lp"] = np.concatenate([g["arc_lp"][:at], np.log(rng.uniform(0.05, 0.95, 300)).astype(np.float32), g["arc_lp"][int(g["arc_ptr"][41]):]])
    g["arc_ptr"] = np.concatenate([g["arc_ptr"][:41], g["arc_ptr"][41:] + 300 - deg[40]]).astype(np.int32)
    g["final_lp"][40] = 0.0
    c = Call().add(AC.scores(70, 19, 12) * SCALE, rng.integers(0, 19, S).tolist(), g).add(AC.scores(5, 19, 13) * SCALE, rng.integers(0, 19, S).tolist(), g)
    want = all_forms(torch, c)
    assert np.isfinite(want[0]).all()


@pytest.mark.parametrize("arcs", (4095, 4096, 4097))
def test_the_arc_staging_cap_at_its_edge(arcs):
    """A segment with one arc fewer than the wave form stages in LDS, exactly as many, and one more (read from the L2 every
    frame), beside a small staged segment in the same launch -- forward over the arcs, backward over the transposed ones."""
    import torch

    assert api.fb_limits()["lds_arcs"] == 4096
    rng = np.random.default_rng(arcs)
    S = 256
    deg = np.full(S, 16)
    deg[0] += arcs - 16 * S
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    assert ptr[-1] == arcs
    src = rng.integers(0, S, arcs).astype(np.int32)
    src[ptr[:-1]] = np.arange(S)  # a self-loop first
    g = dict(states=np.zeros(S, np.int32), arc_ptr=ptr, arc_src=src, arc_lp=np.log(rng.uniform(0.05, 0.95, arcs)).astype(np.float32),
             start_lp=np.zeros(S, np.float32), final_lp=np.zeros(S, np.float32))
    c = Call().add(AC.scores(12, 23, 1) * SCALE, rng.integers(0, 23, S).tolist(), g).add(AC.scores(9, 23, 2) * SCALE, rng.integers(0, 23, 5).tolist(), skip_chain(5, rng))
    want = all_forms(torch, c)
    assert np.isfinite(want[0]).all()


def test_graph_shapes():
    import torch

    ninf = -np.inf
    rows = AC.scores(9, 4, 31) * SCALE
    f32 = lambda *v: np.array(v, np.float32)
    i32 = lambda *v: np.array(v, np.int32)
    # a two-state loop 0 <-> 1 without self-loops, entered in either
    loop = dict(states=i32(0, 0), arc_ptr=i32(0, 1, 2), arc_src=i32(1, 0), arc_lp=f32(-0.5, -0.25), start_lp=f32(0, 0), final_lp=f32(0, 0))
    # backward arcs: 2 -> 0, 3 -> 1 beside the chain
    back = dict(states=i32(0, 0, 0, 0), arc_ptr=i32(0, 2, 5, 7, 9), arc_src=i32(0, 2, 1, 0, 3, 2, 1, 3, 2), arc_lp=f32(-1, -.1, -1, -.2, -.1, -1, -.3, -1, -.1),
                start_lp=None, final_lp=None)
    # several start and final states with different values
    ends = dict(back, start_lp=f32(-2, -0.5, ninf, -1), final_lp=f32(ninf, -1, -0.5, -3))
    # a final state that cannot be reached: state 3 has no arcs and is no start state -- no path, -inf, gamma +0 everywhere
    lost = dict(states=i32(0, 0, 0, 0), arc_ptr=i32(0, 1, 3, 5, 5), arc_src=i32(0, 1, 0, 2, 1), arc_lp=f32(0, 0, 0, 0, 0), start_lp=None, final_lp=None)
    # a state without arcs that is a start state: occupied at t = 0 only
    once = dict(states=i32(0, 0), arc_ptr=i32(0, 0, 2), arc_src=i32(1, 0), arc_lp=f32(-1, -1), start_lp=None, final_lp=None)
    c = Call()
    for g in (loop, back, ends, lost, once):
        c.add(rows[:, :len(g["states"])] if len(g["states"]) < 4 else rows, list(range(len(g["states"]))), g)
    want = all_forms(torch, c)
    b = api.fb_gamma_blocks(want[1], c.T, api.pack_graphs(c.graphs)["statePtr"])
    assert np.isfinite(want[0][:3]).all() and (b[0] > 0).all() and (b[0] < 1).all()  # two alternating paths share the mass
    assert np.isneginf(want[0][3]) and (b[3].view(np.uint32) == 0).all()
    assert np.isfinite(want[0][4]) and (b[4][0] > [0.99, -1]).all() and b[4][0, 1] == 0 and (b[4][1:, 0] == 0).all() and (b[4][1:, 1] > 0.99).all()
    # several finite finals spread over many partials: 600 states, all final, T = 3
    rng = np.random.default_rng(33)
    wide = GC.random_graph(600, rng, starts=40)
    wide["final_lp"] = np.log(rng.uniform(0.05, 0.95, 600)).astype(np.float32)
    d = Call().add(AC.scores(3, 31, 34) * SCALE, rng.integers(0, 31, 600).tolist(), wide)
    want = all_forms(torch, d, wave_launches=(0, 1))
    assert np.isfinite(want[0][0])


def test_the_silence_cases_are_within_the_derived_bound_and_soft():
    """GC.silence_case with halved scores, five seeds in one call: the device's bytes are the restatement's, which is held to
    float64 under the derived bound; the occupancies are soft (tests/test_fb_host.py holds the conditions), and reversing the
    arc order is another input."""
    import torch

    c, r = Call(), Call()
    cases = [FC.soft_silence_case(seed) for seed in range(5)]
    for rows, g, col in cases:
        c.add(rows, col.tolist(), g)
        r.add(rows, col.tolist(), GC.reversed_arcs(g))
    want, rev = all_forms(torch, c), all_forms(torch, r)
    blocks = api.fb_gamma_blocks(want[1], c.T, api.pack_graphs(c.graphs)["statePtr"])
    for s, (rows, g, col) in enumerate(cases):
        te, tb, ge, gb = FC.held(want[0][s], blocks[s], rows[:, col], g)
        print(f"seed {s}: |total - total64| {te:.3g} (bound {tb:.3g}), |gamma - gamma64| {ge:.3g} (bound {gb:.3g})")
        assert te <= tb and ge <= gb and (blocks[s].max(axis=1) < 0.9).mean() >= 0.3
    assert not np.array_equal(want[0].view(np.uint32), rev[0].view(np.uint32))  # the arc order is part of the input


def test_sources_destinations_columns_and_nodes_out_of_range():
    import torch

    lp = LL.priors(WIDTH)
    rng = np.random.default_rng(40)
    chain4 = api.chain_graph([0, 0, 0, 0])
    wide = skip_chain(6, rng)
    c = Call()
    c.add(AC.scores(9, 4, 13) * SCALE, [0, 1, 2, 4], chain4)    # the last state's column at the row stride: no path, -inf, never a NaN
    c.add(AC.scores(9, 4, 14) * SCALE, [0, -1, 2, 3], chain4)   # nothing leaves a NaN
    c.add(AC.scores(9, 6, 15) * SCALE, [0, 1, 7, 3, 4, 5], wide)  # ... but the skip goes round it
    c.add(AC.scores(9, 6, 17) * SCALE, list(range(6)), wide)
    want = all_forms(torch, c)
    b = api.fb_gamma_blocks(want[1], c.T, api.pack_graphs(c.graphs)["statePtr"])
    assert np.isneginf(want[0][:2]).all() and np.isfinite(want[0][2:]).all() and (b[2][:, 2] == 0).all() and (b[0].view(np.uint32) == 0).all()
    # the DEVICE copies hold sources and destinations outside [0, S) while the host tables (which make the plan) are sound:
    # that candidate is a NaN, nothing is read, and the restatement over the same planted tables gives the same bytes
    for bad in (4, -1, 1 << 16, -(1 << 31), 65535):
        d = Call().add(AC.scores(9, 4, 16) * SCALE, [0, 1, 2, 3], chain4).add(AC.scores(9, 6, 17) * SCALE, list(range(6)), wide)
        planted = dict(wide, arc_src=wide["arc_src"].copy())
        planted["arc_src"][int(wide["arc_ptr"][3]) + 1] = bad  # state 3's arc from state 2; the others remain
        d.device_graphs = [dict(chain4, arc_src=np.array([0, 1, bad, 2, 1, 3, 2], np.int32)), planted]
        t = api.fb_transpose(api.pack_graphs(d.graphs))
        t["tSrc"] = t["tSrc"].copy()
        t["tSrc"][[1, 9]] = bad  # two destinations
        d.transposed = t
        want = all_forms(torch, d)
        assert np.isneginf(want[0][0]) and np.isfinite(want[0][1]) and not np.isnan(want[1]).any()
    # a node outside the handle's width: a NaN emission, nothing read
    e = Call()
    for i, nodes in enumerate(([1, 2, 3, WIDTH], [1, -1, 5, 3], [1, 2, 3, 4])):
        e.add(AC.probs(9, 5, 15 + i), [0, 1, 2, 3], chain4, nodes)
    want = all_forms(torch, e, (-20.0, api.LOGLIK_F32), lp)
    assert np.isneginf(want[0][:2]).all() and np.isfinite(want[0][2])


@pytest.mark.parametrize("n_segs,launches", ((1, 1), (2, 1), (64, 1), (65, 2)))
def test_segments_per_launch(n_segs, launches):
    """Segments of unequal T and S, all inside the rule's wave form; 65 need a second launch per direction.  With graphs on
    both sides of the rule's limit every 64 segments go as one launch per form and direction."""
    import torch

    rng = np.random.default_rng(20 + n_segs)
    c = Call()
    for i in range(n_segs):
        S = int(rng.integers(1, 65))
        T = S // 2 + int(rng.integers(1, 40))
        c.add(AC.scores(T, 11, 400 + i) * SCALE, rng.integers(0, 11, S).tolist(), skip_chain(S, rng) if i % 2 else GC.random_graph(S, rng), gap=int(rng.integers(0, 4)))
    want = c.ref()
    got = c.device(torch)
    assert same(got[:2], want) and got[2] == (launches, 0, launches, 0) and np.isfinite(want[0]).sum() >= n_segs // 2
    got = c.device(torch, want_gamma=False)
    assert same(got[:2], c.ref(want_gamma=False)) and got[2] == (launches, 0, 0, 0)
    if n_segs == 2:
        c.add(AC.scores(600, 11, 600) * SCALE, rng.integers(0, 11, 1030).tolist(), skip_chain(1030, rng))
        got = c.device(torch)
        assert same(got[:2], c.ref()) and got[2] == (1, 1, 1, 1)


def test_a_5_state_and_a_1000_state_segment_in_one_launch():
    """The rows of d, the states per lane and the staged arcs are the LAUNCH's largest: a 5-state segment beside a 250-state
    one in the wave form and beside 1000-state ones in the workgroup form; both handles."""
    import torch

    lp = LL.priors(WIDTH)
    for handle in (None, (-20.0, api.LOGLIK_F16)):
        rng = np.random.default_rng(900)
        c = Call()
        for i, (T, S) in enumerate(((20, 5), (300, 1000), (9, 9), (501, 1000), (300, 250))):
            rows = AC.probs(T, 23, 910 + i) if handle is not None else AC.scores(T, 23, 910 + i) * SCALE
            c.add(rows, rng.integers(0, 23, S).tolist(), skip_chain(S, rng), rng.integers(0, WIDTH, S).tolist(), gap=i)
        want = all_forms(torch, c, handle, lp, wave_launches=(1, 1))
        assert np.isfinite(want[0][[0, 2, 3, 4]]).all()


@pytest.mark.parametrize("shift", (1, 2, 3))
def test_row_bases_off_16_bytes(shift):
    import torch

    lp = LL.priors(WIDTH)
    for handle in (None, (-np.inf, api.LOGLIK_F32)):
        c = shaped_call(70, handle, 700 + shift, ld=13, Ts=(90, 50, 117, 3))
        want = c.ref(handle, lp)
        for mode in (1, 2):
            assert same(c.device(torch, handle, lp, mode=mode, shift=shift)[:2], want), (handle, mode)


def test_argument_errors_launch_nothing():
    import torch

    before = api.fb_launches()
    L, i32, i64 = api.lib(), api.C.POINTER(api.C.c_int), api.C.POINTER(api.C.c_longlong)
    buf = torch.zeros(1024, dtype=torch.float32, device="cuda")  # (the one call that launches reads 9 rows of 37 from it)
    p = buf.data_ptr()

    def call(T=(9,), off=(0,), ld=(37,), sp=(0, 5), ap=(0, 1, 2, 3, 4, 5), tp=(0, 1, 2, 3, 4, 5), rows=p, col=p, d_ap=p, d_src=p, d_lp=p, d_tp=p, d_ts=p, d_tl=p,
             total=p, gamma=p, scratch=p, words=45):
        a = [np.array(v, t) for v, t in ((T, np.int32), (off, np.int64), (ld, np.int32), (sp, np.int32))]
        h_ap = None if ap is None else np.array(ap, np.int32).ctypes.data_as(i32)
        h_tp = None if tp is None else np.array(tp, np.int32).ctypes.data_as(i32)
        return L.fdnn_fb_rows_device(None, rows, a[0].ctypes.data_as(i32), a[1].ctypes.data_as(i64), a[2].ctypes.data_as(i32), a[3].ctypes.data_as(i32), h_ap,
                                     h_tp, 1, col, None, d_ap, d_src, d_lp, None, None, d_tp, d_ts, d_tl, scratch, words, total, gamma, None)

    too_many = tuple(np.arange(6) * 40000)  # 200 000 arcs over 5 states
    for bad in (dict(T=(0,)), dict(ld=(0,)), dict(off=(-1,)), dict(sp=(0, 0)), dict(sp=(1, 6)), dict(sp=(0, 16385)), dict(rows=None), dict(col=None),
                dict(total=None), dict(rows=p + 2), dict(gamma=p + 2), dict(scratch=p + 2), dict(words=44), dict(scratch=None),  # (the lattice needs 45 words)
                dict(ap=None), dict(ap=(1, 1, 2, 3, 4, 5)), dict(ap=(0, 2, 1, 3, 4, 5)), dict(ap=too_many), dict(d_ap=None), dict(d_src=None), dict(d_lp=None),
                dict(tp=None), dict(tp=(1, 1, 2, 3, 4, 5)), dict(tp=(0, 2, 1, 3, 4, 5)), dict(tp=(0, 1, 2, 3, 4, 6)), dict(d_tp=None), dict(d_ts=None),
                dict(d_tl=None)):
        assert call(**bad) == api.FDNN_E_ARG, bad
    with pytest.raises(api.FdnnError):
        api.set_fb_kernel(3)
    torch.cuda.synchronize()
    assert api.fb_launches() == before
    assert call(gamma=None, tp=None, d_tp=None, d_ts=None, d_tl=None, scratch=None, words=0) == api.FDNN_OK  # forward only needs none of them
    torch.cuda.synchronize()
    assert tuple(b - a for a, b in zip(before, api.fb_launches())) == (1, 0, 0, 0)
