"""The cases of the forced-alignment tests (tests/test_align_host.py on the CPU, tests/test_gpu_align*.py on the GPU) and the
contract's recursion in numpy, a frame at a time in float32:

    d[0][0] = e(0, 0);  d[0][j] = -inf for j > 0
    stay = d[t-1][j] + self_lp[j];  move = d[t-1][j-1] + next_lp[j-1]  (j = 0: -inf)
    take = move > stay              (false on a tie and for a NaN: stay)
    d[t][j] = (take ? move : stay) + e(t, j);  total = d[T-1][S-1]
    path: j = S-1; for t = T-1 .. 1: path[t] = j; if take[t][j]: j -= 1;  path[0] = j
    total not finite: path is -1 everywhere; a NaN total is 0x7fc00000

Everything is seeded; totals are compared as bits."""
import numpy as np

from fast_dnn_amd import api

QNAN = 0x7fc00000


def align_numpy(e, self_lp=None, next_lp=None):
    """e [T][S] float32 emissions -> (path int32 [T], total bits uint32)."""
    e = np.ascontiguousarray(e, dtype=np.float32)
    T, S = e.shape
    sl = np.zeros(S, np.float32) if self_lp is None else np.asarray(self_lp, np.float32)
    nl = np.zeros(S, np.float32) if next_lp is None else np.asarray(next_lp, np.float32)
    ninf = np.float32(-np.inf)
    d = np.full(S, ninf, np.float32)
    d[0] = e[0, 0]
    takes = np.zeros((T, S), bool)
    with np.errstate(all="ignore"):
        for t in range(1, T):
            stay = d + sl
            move = np.concatenate([[ninf], d[:-1] + nl[:-1]]).astype(np.float32)
            take = move > stay
            takes[t] = take
            d = (np.where(take, move, stay) + e[t]).astype(np.float32)
    total = d[S - 1:S].view(np.uint32)[0]
    if np.isnan(d[S - 1]):
        total = np.uint32(QNAN)
    path = np.full(T, -1, np.int32)
    if np.isfinite(d[S - 1]):
        j = S - 1
        for t in range(T - 1, 0, -1):
            path[t] = j
            j -= int(takes[t, j])
        path[0] = j
    return path, np.uint32(total)


def scores(T, width, seed):
    """Score rows as a decoder sees them: 3 N(0, 1) - 5."""
    return (3 * np.random.default_rng(seed).standard_normal((T, width)) - 5).astype(np.float32)


def probs(T, width, seed):
    """Probability rows: a soft-max of 3 N(0, 1) logits, every value in (0, 1)."""
    z = 3 * np.random.default_rng(seed).standard_normal((T, width))
    p = np.exp(z - z.max(axis=1, keepdims=True))
    return (p / p.sum(axis=1, keepdims=True)).astype(np.float32)


def transitions(S, seed):
    """self_lp = ln U(0.05, 0.95), next_lp = ln(1 - e^self)."""
    u = np.random.default_rng(seed).uniform(0.05, 0.95, S)
    return np.log(u).astype(np.float32), np.log(1 - u).astype(np.float32)


def decoder_case(T, S, seed):
    """ONE generator per seed: the scores 3 N(0, 1) - 5 [T][S] first, then the transitions' uniform draws -> (rows, self_lp,
    next_lp).  (Two generators of the same seed would correlate the scores with the transitions.)"""
    rng = np.random.default_rng(seed)
    rows = (3 * rng.standard_normal((T, S)) - 5).astype(np.float32)
    u = rng.uniform(0.05, 0.95, S)
    return rows, np.log(u).astype(np.float32), np.log(1 - u).astype(np.float32)


def differ(a, b):
    """The fraction of frames in which two paths differ."""
    return float((np.asarray(a) != np.asarray(b)).mean())


def uniform_path(T, S):
    return (np.arange(T, dtype=np.int64) * S // T).astype(np.int32)


def one_segment(rows, col, **kw):
    """api.align_ref of ONE segment whose rows are a [T][ld] array."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    return api.align_ref(rows, [rows.shape[0]], [0], [rows.shape[1]], [0, len(col)], col, **kw)


# ------------------------------------------------------------------------ through the model (tests/test_gpu_align.py and
# tests/test_gpu_signal_nets.py): transcripts from a net's rows and the restatement composed over the lazy sets call's bytes
def transcripts(dense, seg_rows, seed):
    """Per segment: the runs of the rows' argmax, thinned (early runs are kept more often than late ones, so the best path is
    far from the uniform segmentation) and salted with random nodes; S < T, repeats occur."""
    rng = np.random.default_rng(seed)
    O = dense.shape[1]
    ptr, states = [0], []
    for a, b in zip(seg_rows[:-1], seg_rows[1:]):
        best = dense[a:b].argmax(axis=1)
        runs = best[np.concatenate([[True], best[1:] != best[:-1]])]
        keep = rng.random(runs.size) < np.linspace(0.9, 0.05, runs.size)
        keep[0] = True
        st = runs[keep].tolist()
        for _ in range(max(2, (b - a) // 5)):
            st.insert(int(rng.integers(0, len(st) + 1)), int(rng.integers(0, O)))
        st.insert(min(2, len(st)), st[0])  # a repeat
        st = st[:max(1, (b - a) // 2)]
        states.extend(st)
        ptr.append(len(states))
    return np.array(ptr, np.int32), np.array(states, np.int32)


def composed(dnn, x, lp, handle, seg_rows, ptr, states, sl, nl):
    """The restatement over the lazy sets call's bytes -> (path, total)."""
    set_ptr, nodes, col = api.align_sets(ptr, states)
    probs = dnn.calculateLazySets(x, seg_rows, set_ptr, nodes)[0]
    T, ln = np.diff(seg_rows), np.diff(set_ptr)
    off = np.concatenate([[0], np.cumsum(T.astype(np.int64) * ln)[:-1]])
    entry_nodes = np.concatenate([np.tile(nodes[set_ptr[s]:set_ptr[s + 1]], T[s]) for s in range(T.size)])
    e = api.loglik_entries_ref(entry_nodes, probs, lp, handle[0], handle[1]).astype(np.float32)
    return api.align_ref(e, T, off, ln, ptr, col, selfLp=sl, nextLp=nl)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def seg_rows_of(n, n_segs):
    return np.array([0] + [n * (s + 1) // n_segs + (3 if s + 1 < n_segs else 0) for s in range(n_segs)], np.int32)
