"""The fixtures of the list tests (tests/test_lazy_lists_host.py on the CPU, tests/test_gpu_lazy_lists.py on the GPU): for
every case the net, the frames and the masks whose list form is scored, and -- from the oracle alone -- what a list call
must return.  Also a numpy fp32 restatement of the finish kernel's NORMATIVE sum order (fdnn_lists.hip), which the CPU test
holds against the oracle to show that the GPU test's 2e-6 bar is one the order itself can meet.

A case: name -> (net, n, masks builder).  Nets: 'mid' / 'sat' / 'tiny' / 'full' are the suite's session fixtures, anything
else a dispatch_ledger net kind.  Everything is seeded; references are computed once per process (reference())."""
import functools

import numpy as np

import dispatch_ledger as DL
import softmax_ref as SR
from fast_dnn_amd import formats as F

TIGHT = 2e-6  # |p - oracle| per element: the project's soft-max bar
L2E = np.float32(1.44269504088896340736)


def _plant_special_rows(m):
    """Rows 0 .. 3: an empty row, a full row, [0], [O - 1]."""
    m[0] = 0
    m[1] = 1
    m[2] = 0
    m[2, 0] = 1
    m[3] = 0
    m[3, -1] = 1
    return m


def _gen(n, O, share, seed, special=True):
    m = F.generate_masks(n, O, share, 0.03, seed=seed)
    return _plant_special_rows(m) if special and n >= 8 else m


def _full_net_masks(n, O):
    """64 frames of the full net: rows of 8 entries, rows of 1 % (80), and one row that lists every node (the longest chain)."""
    rng = np.random.default_rng(64)
    m = np.zeros((n, O), np.int8)
    for f in range(n):
        m[f, rng.choice(O, 8 if f % 2 == 0 else O // 100, replace=False)] = 1
    m[5] = 1
    return m


def _tail_masks(n, O, kind="tail/ovf"):
    """Half of the rows list the four logits at 95 (they overflow: NaN there, 0 elsewhere), half do not (ordinary rows)."""
    bias = DL._net(kind).layers[-1].bias
    hot = np.nonzero(bias == np.float32(95.0))[0]
    assert hot.size == 4
    m = F.generate_masks(n, O, 0.4, 0.03, seed=95)
    m[:, hot] = 0
    m[::2, hot] = 1
    return m


CASES = {}
for _n in (1, 8, 100, 700):
    for _share in (0.05, 0.40):
        CASES[f"mid.n{_n}.s{int(_share * 100)}"] = ("mid", _n, functools.partial(_gen, _n, 1000, _share, 7 * _n + int(_share * 100)))
CASES["mid.special.n4"] = ("mid", 4, lambda: _plant_special_rows(np.zeros((4, 1000), np.int8)))
CASES["sat.n100.s40"] = ("sat", 100, functools.partial(_gen, 100, 200, 0.40, 21))
CASES["sat.n33.s5"] = ("sat", 33, functools.partial(_gen, 33, 200, 0.05, 22))
CASES["tiny.n100.s40"] = ("tiny", 100, functools.partial(_gen, 100, 100, 0.40, 23))
CASES["tiny.n8.s5"] = ("tiny", 8, functools.partial(_gen, 8, 100, 0.05, 24))
CASES["nosat.n33.s40"] = ("n256/256/nosat", 33, functools.partial(_gen, 33, 256, 0.40, 27))  # no saturating pairs: the walk-free kernel
CASES["odd.lad251.n33"] = ("lad/251", 33, lambda: _odd_masks())
CASES["full.n64"] = ("full", 64, functools.partial(_full_net_masks, 64, 8000))
CASES["rel.lad256.n33.s40"] = ("lad/256", 33, functools.partial(_gen, 33, 256, 0.40, 25, False))
CASES["rel.lad256.n33.full"] = ("lad/256", 33, lambda: np.ones((33, 256), np.int8))
CASES["tail.ovf.n33"] = ("tail/ovf", 33, functools.partial(_tail_masks, 33, 256))

RELATIVE = ("rel.lad256.n33.s40", "rel.lad256.n33.full")  # the cases held to the relative bound


def _odd_masks():
    m = _gen(33, 251, 0.40, 26)
    m[4:, 250] = 1  # node 250: the last one of an odd width, in nearly every list
    return m


def model_path(net, fixtures):
    """fixtures: name -> path of the suite's session fixtures ('mid', 'sat', 'tiny', 'full')."""
    return fixtures[net] if net in fixtures else DL.net_path(net)


def in_dim(net):
    return 432


_REF = {}


def reference(name, fixtures):
    """-> dict(x, masks, row_ptr, nodes, rows (row of every entry), want_probs [nnz], want_inactive [n] (NaN for a full row:
    nothing reads it), acc [nnz], z (the masked fp32 logits [n][O]), want_rows (the oracle's lazy rows [n][O]), orc)"""
    if name in _REF:
        return _REF[name]
    from oracle.oracle import Oracle

    net, n, build = CASES[name]
    masks = np.ascontiguousarray(build(), dtype=np.int8)
    assert masks.shape[0] == n
    x = F.synth_features(n, in_dim(net), seed=900 + len(name) + n)
    orc = Oracle(model_path(net, fixtures))
    hid = orc.hidden_acts_mt(x)
    want_rows = orc.output_mt(hid, masks=masks)
    _, acc = orc.output_mt(hid, want_acc=True)
    row_ptr, nodes = F.masks_to_lists(masks)
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    z = SR.logits(acc, SR.coef_of(orc), orc.layer_bias(orc.n_layers - 1), masks=masks)
    inactive = np.full(n, np.nan, np.float32)
    for f in range(n):
        off = np.nonzero(masks[f] == 0)[0]
        if off.size:
            inactive[f] = want_rows[f, off[0]]
            assert (want_rows[f, off] == inactive[f]).all() or np.isnan(inactive[f])
    _REF[name] = dict(x=x, masks=masks, row_ptr=row_ptr, nodes=nodes, rows=rows, want_probs=want_rows[rows, nodes], want_inactive=inactive,
                      acc=acc[rows, nodes], z=z, want_rows=want_rows, orc=orc, O=masks.shape[1])
    return _REF[name]


def release():
    _REF.clear()


# ------------------------------------------------------------------------------------------- the normative order in numpy
def emulate(z, row_ptr, nodes, O):
    """fp32 restatement of fdnn_lists.hip on exact inputs: e = RN32(2^RN32(z * RN32(log2 e))) (the hardware exp2 idealised as
    correctly rounded), lane l adds e[l], e[l + 64], .. in index order, xor butterfly 32 .. 1, + float(O - len),
    inactive = RN(1 / total), p = RN(e * inactive) -> (probs [nnz], inactive [n])."""
    n = row_ptr.size - 1
    probs = np.zeros(int(row_ptr[-1]), np.float32)
    inactive = np.zeros(n, np.float32)
    lane = np.arange(64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for f in range(n):
            b, e_ = int(row_ptr[f]), int(row_ptr[f + 1])
            y = (z[f, nodes[b:e_]].astype(np.float32) * L2E).astype(np.float32)
            e = np.exp2(y.astype(np.float64)).astype(np.float32)
            s = np.zeros(64, np.float32)
            for i in range(0, e.size, 64):
                part = e[i:i + 64]
                s[:part.size] = (s[:part.size] + part).astype(np.float32)
            for m in (32, 16, 8, 4, 2, 1):
                s = (s + s[lane ^ m]).astype(np.float32)
            total = np.float32(s[0] + np.float32(O - (e_ - b)))
            inv = np.float32(np.float32(1.0) / total)
            inactive[f] = inv
            probs[b:e_] = (e * inv).astype(np.float32)
    return probs, inactive


def depth(length):
    """Rounded additions on the longest path from an entry to its row total: the lane's chain, six butterfly levels, the
    unlisted nodes' term."""
    return max(-(-int(length) // 64) - 1, 0) + 6 + 1


def relative_bound(z_row, listed, p64_row):
    """u (A_i + sum_j p_j A_j + DEPTH + 2) per node of one row; A = 1.23 |z| + c_e('exp2.small') for listed nodes, 0 for the
    others (their e is the exact constant 1)."""
    A = np.where(listed, SR.L_ERR * np.abs(z_row.astype(np.float64)) + SR.C_E_PATH["exp2.small"], 0.0)
    return SR.U * (A + float((p64_row * A).sum()) + depth(int(listed.sum())) + 2)
