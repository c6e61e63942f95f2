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
