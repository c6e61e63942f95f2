"""The cases of the alignment-graph tests (tests/test_align_graph_host.py on the CPU, tests/test_gpu_align_graph*.py on the GPU)
and the contract's recursion in numpy, an arc at a time in float32 (fdnn_align_graph.hpp):

    d[0][j] = start_lp[j] + e(0, j)
    t >= 1: best = -inf, from = -1; for each arc a of j in order: cand = d[t-1][src[a]] + lp[a]; if cand > best: take it
            d[t][j] = best + e(t, j); bp[t][j] = from
    total:  the first of the best d[T-1][j] + final_lp[j], j ascending; not finite: -1 everywhere
    path:   j = end; for t = T-1 .. 1: path[t] = j; j = bp[t][j];  path[0] = j

A graph is a dict (api.chain_graph / api.optional_silence_graph / by hand): states, arc_ptr, arc_src, arc_lp, start_lp,
final_lp.  Everything is seeded; totals are compared as bits."""
import numpy as np

from fast_dnn_amd import api


def graph_numpy(e, g):
    """e [T][S] float32 emissions, g a graph -> (path int32 [T], total bits uint32)."""
    e = np.ascontiguousarray(e, dtype=np.float32)
    T, S = e.shape
    ptr, src, lp = np.asarray(g["arc_ptr"]), np.asarray(g["arc_src"]), np.asarray(g["arc_lp"], np.float32)
    ninf = np.float32(-np.inf)
    start = np.full(S, ninf, np.float32)
    final = np.full(S, ninf, np.float32)
    start[0], final[S - 1] = 0.0, 0.0
    if g.get("start_lp") is not None:
        start = np.asarray(g["start_lp"], np.float32)
    if g.get("final_lp") is not None:
        final = np.asarray(g["final_lp"], np.float32)
    deg = np.diff(ptr)
    bp = np.full((T, S), -1, np.int64)
    with np.errstate(all="ignore"):
        d = (start + e[0]).astype(np.float32)
        for t in range(1, T):
            best = np.full(S, ninf, np.float32)
            frm = np.full(S, -1, np.int64)
            for k in range(int(deg.max()) if deg.size else 0):  # the k-th arc of every state that has one, in list order
                has = np.nonzero(deg > k)[0]
                a = ptr[has] + k
                s = src[a]
                ok = (s >= 0) & (s < S)
                cand = np.where(ok, d[np.where(ok, s, 0)], np.float32(np.nan)).astype(np.float32) + lp[a]
                take = cand > best[has]
                best[has[take]] = cand[take]
                frm[has[take]] = s[take]
            d = (best + e[t]).astype(np.float32)
            bp[t] = frm
        cand = (d + final).astype(np.float32)
    top, end = ninf, -1
    for j in range(S):
        if cand[j] > top:
            top, end = cand[j], j
    path = np.full(T, -1, np.int32)
    if np.isfinite(top):
        j = end
        for t in range(T - 1, 0, -1):
            path[t] = j
            j = int(bp[t, j])
        path[0] = j
    return path, np.array([top], np.float32).view(np.uint32)[0]


def reversed_arcs(g):
    """The same graph with every state's arc list in the opposite order."""
    out = dict(g)
    src, lp = np.array(g["arc_src"], np.int32), np.array(g["arc_lp"], np.float32)
    ptr = np.asarray(g["arc_ptr"])
    for j in range(ptr.size - 1):
        src[ptr[j]:ptr[j + 1]] = src[ptr[j]:ptr[j + 1]][::-1]
        lp[ptr[j]:ptr[j + 1]] = lp[ptr[j]:ptr[j + 1]][::-1]
    out["arc_src"], out["arc_lp"] = src, lp
    return out


def with_scores(g, rng):
    """The same graph with arc scores ln U(0.05, 0.95)."""
    out = dict(g)
    out["arc_lp"] = np.log(rng.uniform(0.05, 0.95, len(g["arc_lp"]))).astype(np.float32)
    return out


def random_graph(S, rng, max_deg=3, integers=False, starts=2, finals=2):
    """In-degrees 0 .. max_deg from any state -- self-loops, forward, skip and backward arcs --, a self-loop first wherever
    there is an arc (so that paths exist at any T), several start and final states."""
    deg = rng.integers(0, max_deg + 1, S)
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    src = rng.integers(0, S, int(ptr[-1])).astype(np.int32)
    src[ptr[:-1][deg > 0]] = np.nonzero(deg > 0)[0]
    lp = rng.integers(-2, 3, src.size).astype(np.float32) if integers else np.log(rng.uniform(0.05, 0.95, src.size)).astype(np.float32)
    start = np.full(S, -np.inf, np.float32)
    final = np.full(S, -np.inf, np.float32)
    start[rng.integers(0, S, starts)] = 0.0
    final[rng.integers(0, S, finals)] = 0.0
    return dict(states=np.zeros(S, np.int32), arc_ptr=ptr, arc_src=src, arc_lp=lp, start_lp=start, final_lp=final)


def ref_one(rows, col, g, **kw):
    """api.align_graph_ref of ONE segment whose rows are a [T][ld] array."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    return api.align_graph_ref(rows, [rows.shape[0]], [0], [rows.shape[1]], api.pack_graphs([g]), col, **kw)


def silence_case(seed, words=6, per_word=6, T=129, width=64, integers=False):
    """A transcript with optional silence on decoder-like scores: `words` words of `per_word` states over distinct columns
    1 .., silence in column 0; scores 3 N(0, 1) - 5 over `width` columns, arc scores ln U(0.05, 0.95) -- or, with integers,
    the scores rounded and zero arc scores (exact sums, many ties) -> (rows [T][width], graph, col [S])."""
    rng = np.random.default_rng(seed)
    rows = (3 * rng.standard_normal((T, width)) - 5).astype(np.float32)
    nodes = [[1 + w * per_word + i for i in range(per_word)] for w in range(words)]
    g = api.optional_silence_graph(nodes, 0)
    if integers:
        rows = np.rint(rows).astype(np.float32)
    else:
        g = with_scores(g, rng)
    return rows, g, np.asarray(g["states"], np.int32)


def silence_states(g):
    return np.nonzero(np.asarray(g["states"]) == 0)[0]
