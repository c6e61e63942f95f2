"""The half net's mid-batch kernel (fdnn_half_mid.hip) under setMid: held to float64 under the bounds of
tests/half_ref.py like the tiled kernel, and to the tiled kernel's BYTES (setMid(0)), as csrc/fdnn_half.hpp's contract asks."""
import numpy as np
import pytest

import float_ref as FR
import half_ref as HR
from fast_dnn_amd import api, formats as F
from test_gpu_half import _load, chain

pytestmark = pytest.mark.gpu

MID = {"mid.sigmoid": 3, "mid.exp": 1, "mid.sigmoid.tap": 3, "mid.exp.tap": 1}
GEMMS = ("hgemm.sigmoid", "hgemm.exp", "hgemm.sigmoid.tap", "hgemm.exp.tap")


def _counts():
    return {**api.half_launches(), **api.half_small_launches(), **api.half_mid_launches()}


@pytest.fixture(scope="module")
def tiny(tmp_models):
    net = F.synth_net([20, 48, 48, 48, 131], seed=21, w0_std=0.05, w_std=0.3)
    dnn = _load(tmp_models, "half_mid_tiny.bin", net)
    x = F.synth_features(300, 20, seed=4, pad_from=None)
    want = dnn.calculate(x)  # the tiled kernel's rows: computed once, shared, never written
    want.setflags(write=False)
    yield dnn, net, x, want
    dnn.delete()


def _both(dnn, net, x, what, mid=4096, small=0):
    before = _counts()
    dnn.setSmall(small), dnn.setMid(mid)
    try:
        got, _ = chain(dnn, net, x, what)
        calc = dnn.calculate(x)
    finally:
        dnn.setSmall(0), dnn.setMid(0)
    return got, calc, {k: v - before[k] for k, v in _counts().items()}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 255, 257, 300])
def test_frames(tiny, n):
    dnn, net, x, want = tiny
    got, calc, d = _both(dnn, net, x[:n], f"mid n {n}")
    assert FR.same_bits(got, want[:n]) and FR.same_bits(calc, want[:n])
    assert {k: d[k] for k in MID} == MID and not any(d[k] for k in GEMMS)


@pytest.mark.parametrize("n,small,mid,takes", [(128, 128, 4096, "small"), (129, 128, 4096, "mid"), (201, 0, 200, "hgemm")])
def test_rule(tiny, n, small, mid, takes):
    """The small kernel keeps its range, the mid kernel takes what lies past it, a call past the mid setting is tiled."""
    dnn, net, x, want = tiny
    got, calc, d = _both(dnn, net, x[:n], f"{takes} n {n}", mid, small)
    assert FR.same_bits(got, want[:n]) and FR.same_bits(calc, want[:n])
    for kind in ("small", "mid", "hgemm"):
        assert [d[f"{kind}.{k}"] for k in ("sigmoid", "exp", "sigmoid.tap", "exp.tap")] == ([3, 1, 3, 1] if kind == takes else [0] * 4), kind


@pytest.mark.parametrize("hidden,out", [(16, 1), (16, 63), (16, 64), (16, 65), (16, 131), (16, 257), (144, 131)])
def test_widths(tmp_models, hidden, out):
    """Output widths around the 64-node partial a workgroup owns; hidden widths 16 and 144 (no multiple of 64); three frame tiles."""
    net = F.synth_net([20, hidden, hidden, hidden, out], seed=7 + out, w0_std=0.05, w_std=0.3)
    dnn = _load(tmp_models, f"half_mid_{hidden}_{out}.bin", net)
    x = F.synth_features(129, 20, seed=6, pad_from=None)
    try:
        want = dnn.calculate(x)
        got, calc, d = _both(dnn, net, x, f"mid {hidden} x {out}")
    finally:
        dnn.delete()
    assert FR.same_bits(got, want) and FR.same_bits(calc, want) and {k: d[k] for k in MID} == MID


@pytest.mark.parametrize("K", [HR.K_LONG, 1552])
def test_long_k(tmp_models, K):
    """The ring (two stages of 128 k) wraps: K = 1040 is 8 full stages and a last one of two MFMA steps, four wraps; K = 1552
    (long_k_case's columns, repeated) is 12 full stages and the same partial one, six wraps.  129 frames: three frame tiles."""
    x, w, b = HR.long_k_case()
    x, w = np.hstack([x, x])[:129, :K], np.hstack([w, w])[:, :K]
    bound, t_min = HR.long_k_margin(x, w, b)
    assert bound < 0.5 * t_min and t_min >= 0.5625
    dims = (20, K, K, K)  # three zero layers in front: the loader wants four, the hidden ones of one width
    zeros = [F.FloatLayerSpec(np.zeros((o, i), np.float32), np.zeros(o, np.float32)) for i, o in zip(dims, dims[1:])]
    net = F.FloatNet(zeros + [F.FloatLayerSpec(w, b)], np.zeros(20, np.float32), np.ones(20, np.float32))
    dnn = _load(tmp_models, f"half_mid_longk_{K}.bin", net)
    try:
        want = dnn.layer(3, x)
        dnn.setMid(4096)
        before = api.half_mid_launches()
        lin, act = dnn.layer(3, x)
        assert api.half_mid_launches()["mid.exp.tap"] == before["mid.exp.tap"] + 1
    finally:
        dnn.delete()
    bad = HR.lin_failures(lin, x, w, b)
    assert not bad.any(), f"{int(bad.sum())} sums outside the float64 bound"
    assert FR.same_bits(lin, want[0]) and FR.same_bits(act, want[1])


def test_rows_stay_in_their_rows(tmp_models):
    """The planted net of test_gpu_half_small at 300 frames (a NaN row, an overflowing logit 7, all-zero rows): every other row
    keeps the clean call's bytes and the whole result is the tiled kernel's, default chunk and chunks of 100, both entry points."""
    import torch

    net = F.synth_net([20, 48, 48, 48, 131], seed=23, w0_std=0.05, w_std=0.3)
    net.layers[0].weights[:, 0] = 1.0
    for l in net.layers[1:3]:
        l.weights[:] = l.weights + np.float32(0.5)
        l.bias[:] = -18.0
    net.layers[3].weights[7, :], net.layers[3].bias[7] = 4.0, -90.0
    dnn = _load(tmp_models, "half_mid_rows.bin", net)
    n = 300
    clean = F.synth_features(n, 20, seed=4, pad_from=None)
    x = clean.copy()
    for first in (0, 100, 200):  # in every chunk of setChunk(100)
        x[first + 5, 3], x[first + 9, 0] = np.nan, 300.0
    x[64], x[299] = 0.0, 0.0
    dirty = np.isin(np.arange(n), [5, 9, 64, 105, 109, 205, 209, 299])
    side = torch.cuda.Stream()
    try:
        for chunk in (0, 100):
            dnn.setChunk(chunk)
            want, want_clean = dnn.calculate(x), dnn.calculate(clean)
            before = api.half_mid_launches()
            dnn.setMid(4096)
            got = dnn.calculate(x)
            assert api.half_mid_launches()["mid.exp"] - before["mid.exp"] == (3 if chunk else 1)
            assert np.isnan(got[5]).all() and np.isnan(got[9, 7]) and (np.delete(got[9], 7) == 0.0).all()
            assert FR.same_bits(got[~dirty], want_clean[~dirty]) and FR.same_bits(got, want), chunk
            xd = torch.from_numpy(x).cuda()
            od = torch.zeros((n, 131), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            dnn.calculateDevice(xd.data_ptr(), n, od.data_ptr(), side.cuda_stream)
            torch.cuda.synchronize()
            assert FR.same_bits(od.cpu().numpy(), want), chunk
            dnn.setMid(0)
    finally:
        dnn.delete()


def test_lazy_sets_ride_along(tiny):
    """calculateLazySets at 300 frames, two segments: the hidden layers take the mid kernel, the bytes stay."""
    dnn, net, x, want = tiny
    tables = ([0, 130, 300], [0, 5, 45], np.concatenate((np.arange(3, 8), np.arange(60, 100))).astype(np.int32))
    want_p, want_i = dnn.calculateLazySets(x, *tables)
    before = api.half_mid_launches()
    dnn.setMid(4096)
    try:
        got_p, got_i = dnn.calculateLazySets(x, *tables)
    finally:
        dnn.setMid(0)
    assert api.half_mid_launches()["mid.sigmoid"] == before["mid.sigmoid"] + 3
    assert FR.same_bits(got_p, want_p) and FR.same_bits(got_i, want_i)


@pytest.mark.parametrize("bad", [-1, 4097])
def test_arguments(tiny, bad):
    dnn, net, x, want = tiny
    dnn.setMid(200)
    try:
        assert api.lib().fdnn_half_model_set_mid(dnn.nativeHandle, bad) == api.FDNN_E_ARG
        before = api.half_mid_launches()
        dnn.calculate(x[:200]), dnn.calculate(x[:201])  # the setting is still 200: one mid call, one tiled
        assert api.half_mid_launches()["mid.exp"] == before["mid.exp"] + 1
    finally:
        dnn.setMid(0)
