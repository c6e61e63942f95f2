"""The planted rows of the top-k tests (tests/test_topk_host.py on the CPU, tests/test_gpu_topk_rows.py on the GPU) and the
contract's selection in numpy: key(v) = u ^ (u >> 31 ? 0xffffffff : 0x80000000), node i before node j when its key is larger
or the keys are equal and i < j.  Everything is seeded; rows are float32 arrays whose BITS matter (NaN payloads, -0)."""
import numpy as np

from fast_dnn_amd import api

WIDTHS = (1, 2, 63, 64, 65, 251, 1001, 8000, api.TOPK_RESIDENT_WIDTH, api.TOPK_RESIDENT_WIDTH + 1)
NS = (1, 5, 130)
KINDS = ("equal", "alternating", "ascending", "descending", "plateau", "special", "softmax")


def ks_for(width):
    top = min(width, api.TOPK_MAX_K)
    return sorted({min(k, top) for k in (1, 2, 63, 64, 65, 256, width)})


def key(rows):
    u = np.ascontiguousarray(rows, dtype=np.float32).view(np.uint32)
    return u ^ np.where(u >> np.uint32(31), np.uint32(0xffffffff), np.uint32(0x80000000))


def select_lexsort(rows, k):
    """The contract, literally: np.lexsort on (index, ~key), the first k -> (nodes int32 [n][k], vals as uint32 [n][k])."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, W = rows.shape
    idx = np.broadcast_to(np.arange(W, dtype=np.int64), (n, W))
    order = np.lexsort((idx, ~key(rows)), axis=-1)[:, :k].astype(np.int32)
    return order, np.take_along_axis(rows.view(np.uint32), order.astype(np.int64), axis=1)


def select(rows, k):
    """The same through one 64-bit word per node, (~key << 32) | index, ascending: a partition for the k smallest, then
    their sort.  The words are distinct, so this IS the lexsort order (tests/test_topk_host.py holds the two together)."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, W = rows.shape
    word = ((~key(rows)).astype(np.uint64) << np.uint64(32)) | np.arange(W, dtype=np.uint64)[None, :]
    if k < W:
        word = np.partition(word, k - 1, axis=1)[:, :k]
    word = np.sort(word, axis=1)
    nodes = (word & np.uint64(0xffffffff)).astype(np.int32)
    return nodes, np.take_along_axis(rows.view(np.uint32), nodes.astype(np.int64), axis=1)


def _bits(values):
    return np.array(values, dtype=np.uint32).view(np.float32)


SPECIALS = _bits([0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001,
                  0x007fffff, 0x807fffff, 0x00800000, 0x3f800000, 0xbf800000, 0x7f7fffff])


def plateau_nodes(width, k):
    """Where a row's ties sit, by row variant: around lane 63 / 64, wave 255 / 256 and the quarter-row chunks of the
    compaction walk, at the first and the last node -- cut down until k - 1 other nodes are left."""
    q = (((width + 3) // 4) + 63) // 64 * 64  # a wave's share of the row (fdnn_topk.hip)
    variants = ([0, width - 1, 62, 63, 64, 65, 255, 256, 257, q - 1, q, 2 * q - 1, 2 * q, 3 * q], [width - 1], [63, 64, 255, 256, q - 1, q],
                [0], [q, width - 1, 3 * q - 1, 3 * q])
    out = []
    for v in variants:
        p = sorted({i for i in v if 0 <= i < width})
        if not p:
            p = [width - 1]
        while width - len(p) < k - 1:
            p.pop(0)
        out.append(np.array(p, dtype=np.int64))
    return out


def rows_of(kind, n, width, k, seed=0):
    """n rows of `width` values of the kind; only 'plateau' depends on k."""
    rng = np.random.default_rng(1000 * width + 7 * len(kind) + seed)
    if kind == "equal":
        return np.full((n, width), 0.25, np.float32)
    if kind == "alternating":
        r = np.where((np.arange(width)[None, :] + np.arange(n)[:, None]) % 2 == 0, np.float32(0.5), np.float32(0.125)).astype(np.float32)
        return np.ascontiguousarray(r)
    if kind in ("ascending", "descending"):
        base = (np.arange(width, dtype=np.float32) + 1.0) / np.float32(width + 1)
        r = np.tile(base if kind == "ascending" else base[::-1], (n, 1)) + (np.arange(n, dtype=np.float32)[:, None] % 4) * np.float32(0.25)
        return np.ascontiguousarray(r, dtype=np.float32)
    if kind == "plateau":
        r = np.full((n, width), 0.0625, np.float32)
        variants = plateau_nodes(width, k)
        for f in range(n):
            p = variants[f % len(variants)]
            r[f, p] = 0.5
            free = np.setdiff1d(np.arange(width), p)
            above = rng.choice(free, k - 1, replace=False)
            r[f, above] = (0.75 + rng.integers(0, 4, k - 1) / 16.0).astype(np.float32)  # four values: ties above the plateau too
        return r
    if kind == "special":
        r = rng.standard_normal((n, width)).astype(np.float32)
        for f in range(n):
            at = rng.integers(0, width, 3 * SPECIALS.size)
            r[f, at] = np.tile(SPECIALS, 3)
        if width >= 2:
            r[0, 0], r[0, -1] = SPECIALS[1], SPECIALS[0]  # -NaN first, +NaN last
        return r
    if kind == "softmax":
        z = (rng.standard_normal((n, width)) * 3.0).astype(np.float32)
        e = np.exp(z - z.max(1, keepdims=True))
        return np.ascontiguousarray((e / e.sum(1, keepdims=True)).astype(np.float32))
    raise KeyError(kind)
