"""The half net's lazy output for per-segment node sets (fdnn_half_set.hip; contract: csrc/fdnn_half_set.hpp): the listed
logits against float64 under half_ref's bound and against the BYTES of the dense kernel's tap, the lazy soft-max against
float64 under half_set_ref's bound, and a row's bytes against every way of reaching them."""
import numpy as np
import pytest

import float_ref as FR
import half_ref as HR
import half_set_ref as HS
from fast_dnn_amd import api, formats as F
from test_gpu_half import _load, chain

pytestmark = pytest.mark.gpu

O = 131
SEG_ROWS = [0, 5, 5, 40, 70, 129]  # an empty segment, boundaries inside a 32-frame tile
SET_LENS = [3, 0, 0, 40, O]


def _counts():
    return {**api.half_launches(), **api.half_small_launches(), **api.half_set_launches()}


def _moved(before):
    return {k: v - before[k] for k, v in _counts().items() if v != before[k]}


def _set(length, seed):
    return np.sort(np.random.default_rng(seed).choice(O, length, replace=False)).astype(np.int32)


@pytest.fixture(scope="module")
def tiny(tmp_models):
    net = F.synth_net([20, 48, 48, 48, O], seed=21, w0_std=0.05, w_std=0.3)
    dnn = _load(tmp_models, "half_set_tiny.bin", net)
    x = F.synth_features(129, 20, seed=4, pad_from=None)
    dense, zd = chain(dnn, net, x, "tiny n 129")  # every layer held to its bounds; computed once, shared, never written
    h = dnn.layer(2, dnn.layer(1, dnn.layer(0, dnn.layer(-1, x)[1])[1])[1])[1]  # the device's own last hidden halves
    assert FR.same_bits(dnn.layer(3, h)[0], zd)
    sets = [_set(length, 50 + s) for s, length in enumerate(SET_LENS)]
    tables = (SEG_ROWS, np.concatenate(([0], np.cumsum(SET_LENS))).astype(np.int32), np.concatenate(sets))
    for a in (dense, zd, h):
        a.setflags(write=False)
    yield dnn, net, x, h, zd, dense, sets, tables
    dnn.delete()


@pytest.mark.parametrize("n", [1, 33, 65, 129])
@pytest.mark.parametrize("length", [1, 31, 32, 33, 64, 65, O])
def test_set_layer(tiny, length, n):
    dnn, net, x, h, zd, dense, _, _ = tiny
    nodes, last = _set(length, length), net.layers[-1]
    before = _counts()
    z, probs, inactive = dnn.setLayer(h[:n], nodes)
    assert _moved(before) == {"set.score.tap": 1}  # and no dense output launch
    bad = HR.lin_failures(z, h[:n], HR.halves(last.weights[nodes]), last.bias[nodes])
    assert not bad.any(), f"{int(bad.sum())} sums outside the float64 bound"
    assert FR.same_bits(z, zd[:n][:, nodes])  # a gathered node sits at its position in the set, not at node mod 32
    HS.check(probs, inactive, z, O, f"len {length} n {n}")
    if length == O:
        assert (np.abs(probs / dense[:n] - 1.0) <= HS.bounds(z, O)[0]).all()


def test_two_frame_tiles_per_fragment(tiny):
    """6600 rows in one chunk: 5 node tiles x 207 frame tiles are more workgroups than the 256 CUs at four tiles each, so a
    workgroup walks five and a W fragment serves two frame tiles (the kernel's FT = 2 form).  A row keeps its bytes."""
    dnn, net, x, h, zd, dense, _, _ = tiny
    assert api.half_set_plan([0, 6600], [0, O], 64, 192)[3] == 5
    nodes, last = np.arange(O, dtype=np.int32), net.layers[-1]
    rows = HR.halves(np.random.default_rng(8).uniform(0.0, 1.0, (6600, 48)))
    rows[:129] = h
    dnn.setChunk(8192)
    try:
        z, probs, inactive = dnn.setLayer(rows, nodes)
        zd_all = dnn.layer(3, rows)[0]
    finally:
        dnn.setChunk(0)
    small = dnn.setLayer(h, nodes)
    assert FR.same_bits(z, zd_all) and all(FR.same_bits(a[:129], b) for a, b in zip((z, probs, inactive), small))
    assert not HR.lin_failures(z, rows, HR.halves(last.weights), last.bias).any()
    HS.check(probs, inactive, z, O, "n 6600")


def test_long_k(tmp_models):
    """K = 1040 (four blocks of the resident tile and a 16-step tail) under long_k_margin's premise: a lost, repeated or skipped
    term, or another node's weights or bias, leaves the bound."""
    x, w, b = HR.long_k_case()
    bound, t_min = HR.long_k_margin(x, w, b)
    assert bound < 0.5 * t_min and t_min >= 0.5625
    dims = (20, HR.K_LONG, HR.K_LONG, HR.K_LONG)
    zeros = [F.FloatLayerSpec(np.zeros((o, i), np.float32), np.zeros(o, np.float32)) for i, o in zip(dims, dims[1:])]
    dnn = _load(tmp_models, "half_set_longk.bin", F.FloatNet(zeros + [F.FloatLayerSpec(w, b)], np.zeros(20, np.float32), np.ones(20, np.float32)))
    nodes = np.sort(np.random.default_rng(3).choice(HR.ROWS_LONG, 37, replace=False)).astype(np.int32)
    try:
        z = dnn.setLayer(x, nodes)[0]
    finally:
        dnn.delete()
    bad = HR.lin_failures(z, x, w[nodes], b[nodes])
    assert not bad.any(), f"{int(bad.sum())} sums outside the float64 bound"


@pytest.mark.parametrize("K,moved", [(384, {"set.score.tap": 1}), (2048, {"set.score.tap": 1}), (2064, {"set.gather": 1, "hgemm.exp.tap": 1})])
def test_k_edge(tmp_models, K, moved):
    """Three k-stages of 128 (an odd count: the last one has no successor to load), the kernel's last width, and the first
    width of the fallback: the dense exp launch and a gather."""
    rng = np.random.default_rng(K)
    dims = (20, K, K, K)
    zeros = [F.FloatLayerSpec(np.zeros((o, i), np.float32), np.zeros(o, np.float32)) for i, o in zip(dims, dims[1:])]
    w, b = HR.halves(rng.normal(0.0, 0.05, (O, K))), rng.normal(0.0, 1.0, O).astype(np.float32)
    dnn = _load(tmp_models, f"half_set_k{K}.bin", F.FloatNet(zeros + [F.FloatLayerSpec(w, b)], np.zeros(20, np.float32), np.ones(20, np.float32)))
    h, nodes = HR.halves(rng.uniform(0.0, 1.0, (33, K))), _set(37, K)
    try:
        zd = dnn.layer(3, h)[0]
        before = _counts()
        z, probs, inactive = dnn.setLayer(h, nodes)
        assert _moved(before) == moved
    finally:
        dnn.delete()
    assert not HR.lin_failures(z, h, w[nodes], b[nodes]).any() and FR.same_bits(z, zd[:, nodes])
    HS.check(probs, inactive, z, O, f"K {K}")


def _per_segment(dnn, rows, sets, call):
    parts = [call(rows[a:b], s) for a, b, s in zip(SEG_ROWS, SEG_ROWS[1:], sets)]
    return np.concatenate([p[-2].ravel() for p in parts]), np.concatenate([p[-1] for p in parts])


@pytest.mark.parametrize("chunk,small", [(0, 0), (32, 0), (0, 128)])
def test_segments(tiny, chunk, small):
    """Every segment's block and inactive values are those of calculateLazySet on its frames alone and of setLayer on its
    last hidden rows, whatever the chunk (a boundary inside a segment) and the small setting; an empty set gives 1 / O."""
    dnn, net, x, h, zd, dense, sets, tables = tiny
    want = _per_segment(dnn, h, sets, dnn.setLayer)
    dnn.setChunk(chunk), dnn.setSmall(small)
    try:
        before = _counts()
        got = dnn.calculateLazySets(x, *tables)
        assert not {"hgemm.exp", "hgemm.exp.tap", "small.exp", "small.exp.tap"} & set(_moved(before))
        alone = _per_segment(dnn, x, sets, dnn.calculateLazySet)
    finally:
        dnn.setChunk(0), dnn.setSmall(0)
    for g, a, w in zip(got, alone, want):
        assert FR.same_bits(g, a) and FR.same_bits(g, w)
    assert FR.same_bits(got[1][5:40], np.full(35, np.float32(1.0) / np.float32(O)))


def test_device_sets_are_not_validated(tiny):
    """Nodes -1 and O in one segment's set: that segment's rows are NaN, every other byte is unchanged, the call returns OK --
    and the host form refuses the same tables."""
    import torch

    dnn, net, x, h, zd, dense, sets, (sr, sp, nodes) = tiny
    want_p, want_i = dnn.calculateLazySets(x, sr, sp, nodes)
    bad = nodes.copy()
    bad[sp[3]], bad[sp[4] - 1] = -1, O
    xd, nd = torch.from_numpy(x).cuda(), torch.from_numpy(bad).cuda()
    pd, idv = torch.zeros(want_p.size, device="cuda"), torch.zeros(129, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    dnn.calculateLazySetsDevice(xd.data_ptr(), 129, sr, sp, nd.data_ptr(), pd.data_ptr(), idv.data_ptr(), side.cuda_stream)
    torch.cuda.synchronize()
    got_p, got_i = pd.cpu().numpy(), idv.cpu().numpy()
    b0, b1 = 5 * 3, 5 * 3 + 30 * 40  # segment 3's block
    assert np.isnan(got_p[b0:b1]).all() and np.isnan(got_i[40:70]).all()
    assert FR.same_bits(np.delete(got_p, np.s_[b0:b1]), np.delete(want_p, np.s_[b0:b1])) and FR.same_bits(np.delete(got_i, np.s_[40:70]), np.delete(want_i, np.s_[40:70]))
    with pytest.raises(api.FdnnError) as e:
        dnn.calculateLazySets(x, sr, sp, bad)
    assert e.value.code == api.FDNN_E_ARG and "segment 3" in str(e.value)


@pytest.mark.parametrize("what", ["rows", "descending", "null"])
def test_arguments(tiny, what):
    dnn, net, x, h, zd, dense, sets, (sr, sp, nodes) = tiny
    if what == "null":
        assert api.lib().fdnn_half_calculate_lazy_sets(None, None, 0, 20, None, None, 0, None, None, None) == api.FDNN_E_ARG
        return
    sr, nodes = list(sr), nodes.copy()
    if what == "rows":
        sr[-1] = 128  # not [0, n)
    else:
        nodes[[0, 1]] = nodes[[1, 0]]
    with pytest.raises(api.FdnnError) as e:
        dnn.calculateLazySets(x, sr, sp, nodes)
    assert e.value.code == api.FDNN_E_ARG
