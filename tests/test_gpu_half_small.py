"""The half net's small-batch kernel (fdnn_half_small.hip): calls of 1 .. 128 frames under setSmall.  Held
to float64 under the bounds of tests/half_ref.py like the tiled kernel, and to the tiled kernel's BYTES: the contract of
csrc/fdnn_half.hpp ("a row's bytes are a function of the row and the model alone") does not know which kernel ran."""
import numpy as np
import pytest

import float_ref as FR
import half_ref as HR
from fast_dnn_amd import api, formats as F
from test_gpu_half import _load, chain

pytestmark = pytest.mark.gpu

SMALL = {"small.sigmoid": 3, "small.exp": 1, "small.sigmoid.tap": 3, "small.exp.tap": 1}
TILED = {"hgemm.sigmoid": 3, "hgemm.exp": 1, "hgemm.sigmoid.tap": 3, "hgemm.exp.tap": 1, "input_step": 2}


@pytest.fixture(scope="module")
def tiny(tmp_models):
    net = F.synth_net([20, 48, 48, 48, 131], seed=21, w0_std=0.05, w_std=0.3)
    dnn = _load(tmp_models, "half_small_tiny.bin", net)
    x = F.synth_features(129, 20, seed=4, pad_from=None)
    want = dnn.calculate(x)  # the tiled kernel's rows: computed once, shared, never written
    want.setflags(write=False)
    yield dnn, net, x, want
    dnn.delete()


def _both(dnn, net, x, what, setting=128):
    """chain and calculate under setSmall(setting) -> (chain's rows, calculate's rows, small deltas, tiled deltas)."""
    before = {**api.half_launches(), **api.half_small_launches()}
    dnn.setSmall(setting)
    try:
        got, _ = chain(dnn, net, x, what)
        calc = dnn.calculate(x)
    finally:
        dnn.setSmall(0)
    d = {k: v - before[k] for k, v in {**api.half_launches(), **api.half_small_launches()}.items()}
    return got, calc, {k: d[k] for k in SMALL}, {k: d[k] for k in TILED}


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 127, 128])
def test_frames(tiny, n):
    dnn, net, x, want = tiny
    got, calc, small, tiled = _both(dnn, net, x[:n], f"small n {n}")
    assert FR.same_bits(got, want[:n]) and FR.same_bits(calc, want[:n])
    assert small == SMALL and tiled == {**dict.fromkeys(TILED, 0), "input_step": 2}


@pytest.mark.parametrize("n,setting", [(129, 128), (33, 32)])
def test_a_call_past_the_setting_is_tiled(tiny, n, setting):
    dnn, net, x, want = tiny
    got, calc, small, tiled = _both(dnn, net, x[:n], f"tiled n {n}", setting)
    assert FR.same_bits(got, want[:n]) and FR.same_bits(calc, want[:n])
    assert small == dict.fromkeys(SMALL, 0) and tiled == TILED


@pytest.mark.parametrize("hidden,out", [(16, 1), (16, 63), (16, 64), (16, 65), (16, 131), (16, 257), (144, 131)])
def test_widths(tmp_models, hidden, out):
    """Output widths around the 64-node partial the output workgroup owns; hidden widths 16 and 144."""
    net = F.synth_net([20, hidden, hidden, hidden, out], seed=7 + out, w0_std=0.05, w_std=0.3)
    dnn = _load(tmp_models, f"half_small_{hidden}_{out}.bin", net)
    x = F.synth_features(33, 20, seed=6, pad_from=None)
    try:
        want = dnn.calculate(x)
        got, calc, small, _ = _both(dnn, net, x, f"small {hidden} x {out}")
    finally:
        dnn.delete()
    assert FR.same_bits(got, want) and FR.same_bits(calc, want) and small == SMALL


@pytest.mark.parametrize("K,n", [(HR.K_LONG, 128), (1552, 32)])
def test_long_k(tmp_models, K, n):
    """The ring wraps.  K = 1040 at 128 frames: a stage of 256 k is 6 tiles of the 9-tile ring, which spans 384 k and wraps
    three times; the last stage is half a step of 32.  At 32 frames a stage is 3 tiles and the ring spans 768 k: K = 1552 is two
    spans and half a step (long_k_case's columns, repeated).  long_k_margin's premise holds for both."""
    x, w, b = HR.long_k_case()
    x, w = np.hstack([x, x])[:n, :K], np.hstack([w, w])[:, :K]
    bound, t_min = HR.long_k_margin(x, w, b)
    print(f"K {K}: bound {bound:.4f}, smallest term {t_min:.4f}")
    assert bound < 0.5 * t_min and t_min >= 0.5625
    dims = (20, K, K, K)  # three zero layers in front: the loader wants four, the hidden ones of one width
    zeros = [F.FloatLayerSpec(np.zeros((o, i), np.float32), np.zeros(o, np.float32)) for i, o in zip(dims, dims[1:])]
    net = F.FloatNet(zeros + [F.FloatLayerSpec(w, b)], np.zeros(20, np.float32), np.ones(20, np.float32))
    dnn = _load(tmp_models, f"half_small_longk_{K}.bin", net)
    try:
        want = dnn.layer(3, x)
        dnn.setSmall(128)
        before = api.half_small_launches()
        lin, act = dnn.layer(3, x)
        assert api.half_small_launches()["small.exp.tap"] == before["small.exp.tap"] + 1
    finally:
        dnn.delete()
    bad = HR.lin_failures(lin, x, w, b)
    assert not bad.any(), f"{int(bad.sum())} sums outside the float64 bound"
    assert FR.same_bits(lin, want[0]) and FR.same_bits(act, want[1])


def test_rows_stay_in_their_rows(tmp_models):
    """A NaN row, a row whose logit 7 overflows (feature 0 = 300 opens every hidden node; logit 7 is 4 sum(a) - 90) and an all-zero
    last row: every other row keeps the clean call's bytes, and the whole result is the tiled kernel's, on every entry point."""
    import torch

    net = F.synth_net([20, 48, 48, 48, 131], seed=23, w0_std=0.05, w_std=0.3)
    net.layers[0].weights[:, 0] = 1.0
    for l in net.layers[1:3]:
        l.weights[:] = l.weights + np.float32(0.5)
        l.bias[:] = -18.0
    net.layers[3].weights[7, :], net.layers[3].bias[7] = 4.0, -90.0
    dnn = _load(tmp_models, "half_small_rows.bin", net)
    clean = F.synth_features(128, 20, seed=4, pad_from=None)
    x = clean.copy()
    for first in (0, 100):  # in both chunks of setChunk(100)
        x[first + 5, 3], x[first + 9, 0] = np.nan, 300.0
    x[32], x[127] = 0.0, 0.0
    dirty = np.isin(np.arange(128), [5, 9, 32, 105, 109, 127])
    side = torch.cuda.Stream()
    try:
        for n, chunk in ((33, 0), (128, 100)):
            dnn.setChunk(chunk)
            want, want_clean = dnn.calculate(x[:n]), dnn.calculate(clean[:n])
            before = api.half_small_launches()
            dnn.setSmall(128)
            got = dnn.calculate(x[:n])
            assert api.half_small_launches()["small.exp"] - before["small.exp"] == (2 if chunk else 1)
            assert np.isnan(got[5]).all() and np.isnan(got[9, 7]) and (np.delete(got[9], 7) == 0.0).all()
            assert FR.same_bits(got[~dirty[:n]], want_clean[~dirty[:n]]) and FR.same_bits(got, want), (n, chunk)
            xd = torch.from_numpy(x[:n]).cuda()
            od = torch.zeros((n, 131), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            dnn.calculateDevice(xd.data_ptr(), n, od.data_ptr(), side.cuda_stream)
            torch.cuda.synchronize()
            assert FR.same_bits(od.cpu().numpy(), want), (n, chunk)
            dnn.setSmall(0)
    finally:
        dnn.delete()


@pytest.mark.parametrize("bad", [-1, 129])
def test_arguments(tiny, bad):
    dnn, net, x, want = tiny
    dnn.setSmall(32)
    try:
        assert api.lib().fdnn_half_model_set_small(dnn.nativeHandle, bad) == api.FDNN_E_ARG
        before = api.half_small_launches()
        dnn.calculate(x[:32]), dnn.calculate(x[:33])  # the setting is still 32: one small call, one tiled
        assert api.half_small_launches()["small.exp"] == before["small.exp"] + 1
    finally:
        dnn.setSmall(0)
