"""The fixtures of the set tests (tests/test_lazy_set_host.py on the CPU, tests/test_gpu_lazy_set.py on the GPU): for every
case the net, the context's frames, the node set and the row ranges (first, count) that are scored with it, and -- from the
oracle alone, as lazy_lists_cases.reference does, the mask being the set in every row -- what a set call must return.

A case: name -> Case(net, n, nodes builder, ranges).  Nets as in lazy_lists_cases.  NT and FT are the set kernel's node and
frame tile (api.SET_NODE_TILE, api.SET_FRAME_TILE: fdnn_set.hpp's constants)."""
import collections

import numpy as np

import dispatch_ledger as DL
import lazy_lists_cases as LC
import softmax_ref as SR
from fast_dnn_amd import api, formats as F

NT, FT = api.SET_NODE_TILE, api.SET_FRAME_TILE
TIGHT = LC.TIGHT

Case = collections.namedtuple("Case", "net n O build ranges")


def pick(O, length, seed, must=()):
    """`length` nodes of [0, O), ascending, with the nodes of `must` among them."""
    rng = np.random.default_rng(seed)
    must = np.array(sorted(set(must)), np.int32)[:length]
    rest = np.setdiff1d(np.arange(O, dtype=np.int32), must)
    more = rng.choice(rest, length - must.size, replace=False).astype(np.int32)
    return np.sort(np.concatenate((must, more))).astype(np.int32)


def _hot(kind):
    return np.nonzero(DL._net(kind).layers[-1].bias == np.float32(95.0))[0].astype(np.int32)


COUNTS = (1, FT - 1, FT + 1, 100)
CASES = {}
for _len in (0, 1, NT - 1, NT, NT + 1, 2 * NT + 1, 1000):  # every set with node 0 and node O - 1 (len 1: node 0)
    CASES[f"mid.len{_len}"] = Case("mid", 100, 1000, (lambda L=_len: pick(1000, L, 10 + L, (0, 999))), tuple((0, c) for c in COUNTS))
CASES["mid.last"] = Case("mid", 100, 1000, lambda: np.array([999], np.int32), ((0, FT + 1),))
CASES["mid.first7"] = Case("mid", 100, 1000, lambda: pick(1000, NT + 1, 77, (0, 999)), ((7, FT + 1), (7, 93)))
CASES["sat.len10"] = Case("sat", 33, 200, lambda: pick(200, 10, 21, (0, 199)), ((0, 33),))
CASES["sat.len200"] = Case("sat", 33, 200, lambda: pick(200, 200, 22), ((0, 33),))
CASES["nosat.len100"] = Case("n256/256/nosat", 33, 256, lambda: pick(256, 100, 27, (0, 255)), ((0, 33),))  # the walk-free instance
CASES["odd.lad251"] = Case("lad/251", 33, 251, lambda: pick(251, 70, 26, (250,)), ((0, 33),))  # an odd width, its last node
CASES["tiny.len40"] = Case("tiny", 33, 100, lambda: pick(100, 40, 23, (0, 99)), ((0, 33),))
for _len in (8, 80, 8000):  # K = 2048, and the longest chain of the row sum
    CASES[f"full.len{_len}"] = Case("full", 64, 8000, (lambda L=_len: pick(8000, L, 64 + L, (0, 7999))), ((0, 64),))
CASES["rel.lad256.len100"] = Case("lad/256", 33, 256, lambda: pick(256, 100, 25, (0, 255)), ((0, 33),))
CASES["rel.lad256.full"] = Case("lad/256", 33, 256, lambda: np.arange(256, dtype=np.int32), ((0, 33),))
CASES["tail.ovf.hot"] = Case("tail/ovf", 33, 256, lambda: pick(256, 100, 95, _hot("tail/ovf")), ((0, 33),))  # the four logits at 95 listed
CASES["tail.ovf.cold"] = Case("tail/ovf", 33, 256,
                              lambda: np.setdiff1d(pick(256, 104, 96), _hot("tail/ovf")).astype(np.int32), ((0, 33),))
CASES["k2304.len70"] = Case("k2304", 33, 252, lambda: pick(252, 70, 61, (0, 251)), ((0, 33),))  # K > 2048: served by the list kernels

RELATIVE = ("rel.lad256.len100", "rel.lad256.full")
TAIL = ("tail.ovf.hot", "tail.ovf.cold")
FALLBACK_BY_SHAPE = ("k2304.len70",)  # the MFMA kernel's shape does not apply (fdnn_set.hpp: shape_applies)

_NET = {}  # (net, n) -> x, oracle, hidden activations, dense accumulators
_REF = {}


def _net_ref(net, n, fixtures):
    if (net, n) not in _NET:
        from oracle.oracle import Oracle

        orc = Oracle(LC.model_path(net, fixtures))
        x = F.synth_features(n, LC.in_dim(net), seed=1300 + n + len(net))
        hid = orc.hidden_acts_mt(x)
        _, acc = orc.output_mt(hid, want_acc=True)
        _NET[(net, n)] = (x, orc, hid, acc)
    return _NET[(net, n)]


def reference(name, fixtures):
    """-> dict(x [n][D], nodes [len], O, acc [n][len], z (the masked fp32 logits [n][O]), masks [n][O], want_rows (the oracle's
    lazy rows [n][O]), want_probs [n][len], want_inactive [n] (NaN where every node is listed: nothing reads it), and the
    set as uniform lists over all n rows: row_ptr [n + 1], list_nodes [n * len])"""
    if name in _REF:
        return _REF[name]
    c = CASES[name]
    x, orc, hid, acc = _net_ref(c.net, c.n, fixtures)
    nodes = np.ascontiguousarray(c.build(), dtype=np.int32)
    assert nodes.ndim == 1 and (np.diff(nodes) > 0).all() and (nodes.size == 0 or (nodes[0] >= 0 and nodes[-1] < c.O))
    masks = np.zeros((c.n, c.O), np.int8)
    masks[:, nodes] = 1
    want_rows = orc.output_mt(hid, masks=masks)
    assert want_rows.shape == (c.n, c.O)
    z = SR.logits(acc, SR.coef_of(orc), orc.layer_bias(orc.n_layers - 1), masks=masks)
    off = np.setdiff1d(np.arange(c.O), nodes)
    inactive = want_rows[:, off[0]].copy() if off.size else np.full(c.n, np.nan, np.float32)
    if off.size:
        assert all(((want_rows[f, off] == inactive[f]) | np.isnan(inactive[f])).all() for f in range(c.n))
    _REF[name] = dict(x=x, nodes=nodes, O=c.O, acc=acc[:, nodes], z=z, masks=masks, want_rows=want_rows, want_probs=want_rows[:, nodes],
                      want_inactive=inactive, row_ptr=uniform_row_ptr(c.n, nodes.size), list_nodes=np.tile(nodes, c.n))
    return _REF[name]


def uniform_row_ptr(count, length):
    return (np.arange(count + 1, dtype=np.int64) * length).astype(np.int32)


def release():
    _REF.clear()
    _NET.clear()
