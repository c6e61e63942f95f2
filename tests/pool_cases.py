"""The maps of the class-pooling tests (tests/test_pool_host.py on the CPU, tests/test_gpu_pool*.py on the GPU) and the
contract's sum in numpy, stated independently of fdnn_pool.hpp: for a class with members m_0 < m_1 < ... < m_{L-1}

    s_j = +0;  for t = j, j + 16, ...: s_j = s_j + p[m_t]      (j = 0 .. lanes - 1)
    q   = the pairwise tree (s_0+s_1), ((s_0+s_1)+(s_2+s_3)), ... over the lanes

every + one float32 addition.  The number of partial sums is read from the library (api.pool_limits()), never written here.
Everything is seeded; rows are float32 arrays whose BITS matter (-0, denormals, inf, NaN)."""
import numpy as np

from fast_dnn_amd import api

SIZES = (0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257)  # class sizes around one, two and sixteen steps of the sixteen lanes
MAP_KINDS = ("one", "identity", "interleaved", "blocks", "giant", "sizes", "gaps", "quarter_out", "none")
U = 2.0 ** -24


def lanes():
    return api.pool_limits()[0]


def map_of(kind, width, seed=0, classes=None):
    """(class_of int32 [width], n_classes) of the kind at this width (classes: how many an `interleaved` map has, 48 unless given)."""
    rng = np.random.default_rng(77 * width + 13 * len(kind) + seed)
    i = np.arange(width, dtype=np.int64)
    if kind == "one":
        return np.zeros(width, np.int32), 1
    if kind == "identity":
        return i.astype(np.int32), width
    if kind == "interleaved":
        C = min(width, classes or 48)
        return (i % C).astype(np.int32), C
    if kind == "blocks":  # contiguous, uneven blocks
        C = min(width, 5)
        return np.minimum(i * C // width, C - 1).astype(np.int32), C
    if kind == "giant":  # one giant class and singletons at both ends
        C = min(width, 4)
        co = np.zeros(width, np.int32)
        if C > 1:
            co[0] = 1
        for c in range(2, C):
            co[width - 1 - (c - 2)] = c
        return co, C
    if kind == "sizes":  # classes of the listed sizes (as many as fit), members scattered over the row, the rest in no class
        co = np.full(width, -1, np.int32)
        order = rng.permutation(width)
        at = 0
        sizes = []
        for s in SIZES:
            if at + s > width or len(sizes) + 1 > width:
                break
            co[order[at:at + s]] = len(sizes)
            sizes.append(s)
            at += s
        return co, max(len(sizes), 1)
    if kind == "gaps":  # empty classes between full ones
        C = min(width, 7)
        return (2 * (i % ((C + 1) // 2))).astype(np.int32), C
    if kind == "quarter_out":
        C = min(width, 11)
        co = (i % C).astype(np.int32)
        co[rng.permutation(width)[:width // 4]] = -1
        return co, C
    if kind == "none":
        return np.full(width, -1, np.int32), min(width, 3)
    raise KeyError(kind)


def members(class_of, n_classes):
    co = np.asarray(class_of)
    return [np.nonzero(co == c)[0] for c in range(n_classes)]


def pool_numpy(rows, class_of, n_classes):
    """The rule, vectorised over rows and lanes: float32 [n][C].  Padding a class to whole steps with +0 changes nothing: a
    partial sum starts at +0 and can never be -0 (x + y is -0 only for -0 + -0), so s + (+0) returns s's own bits."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, L = rows.shape[0], lanes()
    out = np.zeros((n, n_classes), np.float32)
    with np.errstate(all="ignore"):
        for c, m in enumerate(members(class_of, n_classes)):
            steps = -(-m.size // L)
            v = np.zeros((n, steps * L), np.float32)
            v[:, :m.size] = rows[:, m]
            v = v.reshape(n, steps, L)
            s = np.zeros((n, L), np.float32)
            for t in range(steps):
                s = s + v[:, t, :]
            while s.shape[1] > 1:
                s = s[:, 0::2] + s[:, 1::2]
            out[:, c] = s[:, 0]
    return out


def pool_literal(row, member):
    """One class of one row, scalar by scalar as the contract writes it."""
    L = lanes()
    with np.errstate(all="ignore"):
        s = [np.float32(0.0)] * L
        for j in range(L):
            for t in range(j, len(member), L):
                s[j] = np.float32(s[j] + np.float32(row[member[t]]))
        d = 1
        while d < L:
            for j in range(0, L, 2 * d):
                s[j] = np.float32(s[j] + s[j + d])
            d *= 2
    return s[0]


def depth(size):
    return -(-size // lanes()) + 4


def oracle_bound(size, exact, bar):
    """The allowed |q_c - exact| of a class of `size` members against the float64 sum `exact` of the oracle's probabilities:
    the absolute bar per probability plus the derived bound of the additions, d u / (1 - d u) (exact + size bar), d = depth(size)."""
    d = depth(size)
    return size * bar + d * U / (1 - d * U) * (exact + size * bar)


def same_bytes(got, want):
    """Byte for byte, NaN against NaN (payloads are the hardware's business) -> bool."""
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if g.shape != w.shape:
        return False
    gn, wn = np.isnan(g), np.isnan(w)
    return bool(np.array_equal(gn, wn) and np.array_equal(g.view(np.uint32)[~gn], w.view(np.uint32)[~wn]))
