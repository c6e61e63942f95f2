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

import align_cases as AC
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


# ------------------------------------------------------------------ through the model (tests/test_gpu_align_graph.py and
# tests/test_gpu_signal_nets.py): optional-silence transcripts from a net's rows, the restatement composed over the lazy sets
# call's bytes, and the condition under which the comparison is not blind
FAR = -1000.0  # an arc score no emission makes up for (the handles' floor is -20)


def silence_node(dense):
    """The node that is the argmax of the most rows: a silence that the scores do favour on some frames."""
    return int(np.bincount(dense.argmax(axis=1)).argmax())


def silence_graphs(dense, seg_rows, seed, words_per_seg=None):
    """Per segment an optional-silence transcript: the silence is silence_node(dense), the words are three states each from the
    runs of the rows' argmax without the silence (padded with random nodes), arc scores ln U(0.05, 0.95).  So that the
    comparison is not blind whatever the scores say, entering the silence after word 0 costs FAR (it is SKIPPED) and so does
    the skip over the silence after word 1 (that silence is TAKEN); every other silence is left to the scores."""
    rng = np.random.default_rng(seed)
    O, sil = dense.shape[1], silence_node(dense)
    graphs = []
    for a, b in zip(seg_rows[:-1], seg_rows[1:]):
        best = dense[a:b].argmax(axis=1)
        runs = [int(v) for v in best[np.concatenate([[True], best[1:] != best[:-1]])] if v != sil]
        n_words = words_per_seg or max(3, (b - a) // 12)
        pad = [int(v) if v != sil else (int(v) + 1) % O for v in rng.integers(0, O, max(0, 3 * n_words - len(runs)))]
        nodes = runs[:3 * n_words] + pad
        words = [nodes[3 * w:3 * w + 3] for w in range(n_words)]
        g = api.optional_silence_graph(words, sil)
        g["arc_lp"] = np.log(rng.uniform(0.05, 0.95, g["arc_lp"].size)).astype(np.float32)
        ptr = g["arc_ptr"]
        g["arc_lp"][ptr[4] + 1] = FAR  # state 4 = the silence after word 0: its arc from word 0's last state
        g["arc_lp"][ptr[9] + 1] = FAR  # state 9 = word 2's first state: its arc from word 1's last state, the skip
        graphs.append(g)
    return graphs


def composed(dnn, x, lp, handle, seg_rows, packed):
    """The restatement over the lazy sets call's bytes -> (path, total)."""
    ptr, states = packed["statePtr"], packed["states"]
    set_ptr, nodes, col = api.align_sets(ptr, states)
    probs = dnn.calculateLazySets(x, seg_rows, set_ptr, nodes)[0]
    T, ln = np.diff(seg_rows), np.diff(set_ptr)
    off = np.concatenate([[0], np.cumsum(T.astype(np.int64) * ln)[:-1]])
    entry_nodes = np.concatenate([np.tile(nodes[set_ptr[s]:set_ptr[s + 1]], T[s]) for s in range(T.size)])
    e = api.loglik_entries_ref(entry_nodes, probs, lp, handle[0], handle[1]).astype(np.float32)
    return api.align_graph_ref(e, T, off, ln, packed, col), (e, T, off, ln, col)


def not_blind(net, want, pieces, seg_rows, graphs):
    """On the restatement alone: the paths take some silences and skip others, and differ from the forced-silence chain's.
    Silences 4 and 8 are planted; what the scores decide about the others is printed."""
    e, T, off, ln, col = pieces
    sp = np.concatenate([[0], np.cumsum([len(g["states"]) for g in graphs])]).astype(np.int32)
    chain = api.align_ref(e, T, off, ln, sp, col)  # every silence forced: the chain over the same states
    for s, g in enumerate(graphs):
        p = want[0][seg_rows[s]:seg_rows[s + 1]]
        sil = np.arange(0, len(g["states"]), 4)  # the silence before each three-state word and the one after the last
        took = [int(j) for j in sil if (p == j).any()]
        frac = AC.differ(p, chain[0][seg_rows[s]:seg_rows[s + 1]])
        print(f"{net} segment {s}: T {p.size} S {len(g['states'])}, silences taken {took} of {sil.tolist()}, {frac:.0%} of the frames off the forced-silence chain")
        assert 8 in took and 4 not in took and 0 < len(took) < sil.size and frac > 0
