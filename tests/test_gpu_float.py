"""The unquantized net on the device (fdnn_float.hip) against its host restatement, byte for byte, and against float64
within the bounds of tests/float_ref.py: every layer judged alone, on the fp32 inputs the device was given.

  1  lin == fdnn_debug_float_layer_ref, bit for bit (input step included)      2  lin within gamma(K + 1) (...) of float64
  3  sigmoid within u (sigma (1 - sigma) (1.23 |z| + c_e) + 3)                  4  soft-max within softmax_ref's relative bound
  5  a row's bytes do not depend on the batch, the position, the chunk or the entry point
"""
import os

import numpy as np
import pytest

import float_ref as FR
import softmax_ref as SR
from fast_dnn_amd import api, convert as CV, formats as F

pytestmark = pytest.mark.gpu

TIGHT = 2e-6  # the suite's absolute bar on a probability


def _load(tmp_models, name, net):
    p = os.path.join(tmp_models, name)
    F.write_model_bin(p, net)
    return api.FloatDnn.loadFromFile(p, device=0)


def _soft_max_checks(probs, z, rows, what):
    SR.check(probs, z, SR.rows_pad_of(rows), what, c_e=FR.C_E)
    assert np.abs(probs.astype(np.float64) - SR.softmax64(z)).max() <= TIGHT, what


def chain(dnn, net, x, what, soft_max=True):
    """The net layer by layer through fdnn_debug_float_layer, each layer held to items 1-4 -> (probabilities, logits)."""
    lin, cur = dnn.layer(-1, x)
    rl, ra = api.float_input_ref(net.shift, net.scale, x)
    assert FR.same_bits(lin, rl) and FR.same_bits(cur, ra), f"{what}: input step differs from the restatement"
    last = len(net.layers) - 1
    for j, l in enumerate(net.layers):
        lin, act = dnn.layer(j, cur)
        assert FR.same_bits(lin, api.float_layer_ref(l.weights, l.bias, cur)), f"{what}: layer {j} sums differ from the restatement"
        bad = FR.lin_failures(lin, cur, l.weights, l.bias)
        assert not bad.any(), f"{what}: layer {j}: {int(bad.sum())} sums outside the float64 bound"
        if j < last:
            bad = FR.sigmoid_failures(act, lin)
            assert not bad.any(), f"{what}: layer {j}: {int(bad.sum())} sigmoids outside the bound"
        elif soft_max:
            _soft_max_checks(act, lin, l.out_dim, f"{what}: soft-max")
        cur = act
    return cur, lin


# ------------------------------------------------------------------------------------------------ tiny net 20 -> 3 x 48 -> 131
@pytest.fixture(scope="module")
def tiny(tmp_models):
    net = F.synth_net([20, 48, 48, 48, 131], seed=21, w0_std=0.05, w_std=0.3)
    dnn = _load(tmp_models, "float_tiny.bin", net)
    x = F.synth_features(300, 20, seed=4, pad_from=None)
    want, _ = chain(dnn, net, x, "tiny n 300")  # computed once, shared, never written
    want.setflags(write=False)
    yield dnn, net, x, want
    dnn.delete()


def test_tiny_shape(tiny):
    dnn = tiny[0]
    assert (dnn.inputDimension(), dnn.outputDimension(), dnn.layerCount()) == (20, 131, 4)
    assert [dnn.layerDimension(j) for j in range(4)] == [48, 48, 48, 131] and dnn.layerDimension(4) == -1 and dnn.device() == 0
    with pytest.raises(ValueError):
        dnn.calculate(np.zeros((2, 19), np.float32))
    assert api.lib().fdnn_debug_float_layer(dnn.nativeHandle, 4, None, 1, None, None) == api.FDNN_E_ARG  # layer index out of range
    assert api.lib().fdnn_debug_float_layer(dnn.nativeHandle, 0, None, 1, None, None) == api.FDNN_E_ARG  # null buffer
    assert api.lib().fdnn_float_calculate(dnn.nativeHandle, None, 1, 20, None) == api.FDNN_E_ARG
    assert dnn.calculate(np.zeros((0, 20), np.float32)).shape == (0, 0)
    # the measurement twin of the per-layer call: a time, and no layer -1
    h = np.full((130, 48), 0.5, np.float32)
    assert dnn.layerMicros(1, h, reps=2) > 0.0 and dnn.layerMicros(3, h, reps=1) > 0.0
    with pytest.raises(api.FdnnError) as e:
        dnn.layerMicros(-1, np.zeros((2, 20), np.float32))
    assert e.value.code == api.FDNN_E_ARG


@pytest.mark.parametrize("n", [1, 127, 128, 129, 300])
def test_tiny_every_layer(tiny, n):
    dnn, net, x, want = tiny
    before = api.float_launches()
    got, _ = chain(dnn, net, x[:n], f"tiny n {n}")
    assert FR.same_bits(got, want[:n])  # item 5: the batch
    assert FR.same_bits(dnn.calculate(x[:n]), want[:n])  # the composition of the per-layer calls
    after = api.float_launches()
    # per instance: the chain runs the tap forms (3 hidden + 1 output), calculate the plain ones; one input step each
    assert after["fgemm.sigmoid.tap"] - before["fgemm.sigmoid.tap"] == 3 and after["fgemm.exp.tap"] - before["fgemm.exp.tap"] == 1
    assert after["fgemm.sigmoid"] - before["fgemm.sigmoid"] == 3 and after["fgemm.exp"] - before["fgemm.exp"] == 1
    assert after["input_step"] - before["input_step"] == 2


def test_tiny_rows_do_not_depend_on_batch_position_chunk_or_entry_point(tiny):
    import torch

    dnn, net, x, want = tiny
    for n, first in ((1, 0), (1, 299), (33, 100), (129, 171), (300, 0)):
        assert FR.same_bits(dnn.calculate(x[first:first + n]), want[first:first + n]), (n, first)
    perm = np.random.default_rng(1).permutation(300)
    assert FR.same_bits(dnn.calculate(x[perm]), want[perm])
    xd = torch.from_numpy(x).cuda()
    try:
        for chunk in (128, 160, 0):
            dnn.setChunk(chunk)
            assert FR.same_bits(dnn.calculate(x), want), chunk
            od = torch.zeros((300, 131), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            dnn.calculateDevice(xd.data_ptr(), 300, od.data_ptr(), 0)
            torch.cuda.synchronize()
            assert FR.same_bits(od.cpu().numpy(), want), chunk
            lin, act = dnn.layer(3, dnn.layer(2, dnn.layer(1, dnn.layer(0, dnn.layer(-1, x)[1])[1])[1])[1])
            assert FR.same_bits(act, want), chunk
        side = torch.cuda.Stream()
        od = torch.zeros((300, 131), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dnn.calculateDevice(xd.data_ptr(), 300, od.data_ptr(), side.cuda_stream)
        side.synchronize()
        assert FR.same_bits(od.cpu().numpy(), want)
    finally:
        dnn.setChunk(0)
    with pytest.raises(api.FdnnError):
        dnn.setChunk(-1)


def test_tiny_across_the_default_chunk_boundary(tiny):
    """4100 frames: the default chunk (4096) is crossed on the device, the second chunk has 4 frames."""
    dnn, net, x, want = tiny
    idx = np.arange(4100) % 300
    before = api.float_launches()
    got = dnn.calculate(x[idx])
    after = api.float_launches()
    assert FR.same_bits(got, want[idx])
    assert after["input_step"] - before["input_step"] == 2 and after["fgemm.exp"] - before["fgemm.exp"] == 2


def test_a_nan_in_x_stays_in_its_row(tiny):
    dnn, net, x, want = tiny
    xn = x[:130].copy()
    xn[77, 5] = np.nan
    got = dnn.calculate(xn)
    assert np.isnan(got[77]).all()
    keep = np.arange(130) != 77
    assert FR.same_bits(got[keep], want[:130][keep])


# ------------------------------------------------------------------------------------------------ the long-k layer
def test_long_k_layer(tmp_models):
    """K = 2064: 64 k-steps plus half a step; every term in [0.5625, 1] so that ONE lost or repeated term leaves bound 2."""
    x, w, b = FR.long_k_case()
    K, rows = FR.K_LONG, FR.ROWS_LONG
    zeros = F.FloatLayerSpec(np.zeros((K, K), np.float32), np.zeros(K, np.float32))
    net = F.FloatNet([F.FloatLayerSpec(np.zeros((K, 20), np.float32), np.zeros(K, np.float32)), zeros, zeros, F.FloatLayerSpec(w, b)],
                     np.zeros(20, np.float32), np.ones(20, np.float32))
    dnn = _load(tmp_models, "float_longk.bin", net)
    try:
        lin, _ = dnn.layer(3, x)
    finally:
        dnn.delete()
    assert FR.same_bits(lin, api.float_layer_ref(w, b, x))
    bad = FR.lin_failures(lin, x, w, b)
    assert not bad.any(), f"{int(bad.sum())} sums outside the float64 bound"


# ------------------------------------------------------------------------------------------------ wide net 432 -> 3 x 256 -> 1000
def test_wide_net_end_to_end(tmp_models):
    net = F.synth_net([432, 256, 256, 256, 1000], seed=5)
    dnn = _load(tmp_models, "float_wide.bin", net)
    x = F.synth_features(300, 432, seed=3)
    try:
        want, z = chain(dnn, net, x, "wide")
        got = dnn.calculate(x)
    finally:
        dnn.delete()
    assert FR.same_bits(got, want)
    p64 = SR.softmax64(z)
    slack = (p64 * SR.bound(z, p64, SR.rows_pad_of(1000), FR.C_E)).sum(axis=1)
    assert (np.abs(got.astype(np.float64).sum(axis=1) - 1.0) <= slack).all()
    host = CV.float_forward(net, x)  # numpy's blocked order: not a bar
    print(f"wide net: max |device - convert.float_forward| = {np.abs(got - host).max():.3e}")


# ------------------------------------------------------------------------------------------------ ends of the range
def _ends_net():
    return F.synth_net([20, 48, 48, 48, 131], seed=23)


def test_sigmoid_ends_are_exact(tmp_models):
    net = _ends_net()
    b = net.layers[1].bias
    b[0::2], b[1::2] = 120.0, -120.0
    dnn = _load(tmp_models, "float_ends_sig.bin", net)
    x = F.synth_features(33, 20, seed=6, pad_from=None)
    try:
        cur = dnn.layer(0, dnn.layer(-1, x)[1])[1]
        lin, act = dnn.layer(1, cur)
        probs = dnn.calculate(x)
    finally:
        dnn.delete()
    assert (lin[:, 0::2] > 104).all() and (lin[:, 1::2] < -89).all()
    assert (act[:, 0::2] == 1.0).all() and (act[:, 1::2] == 0.0).all() and not np.signbit(act).any()
    assert np.isfinite(probs).all()


def test_an_overflowing_logit_is_nan_and_the_rest_zero(tmp_models):
    net = _ends_net()
    net.layers[3].weights[:] = (net.layers[3].weights * np.float32(0.01)).astype(np.float32)
    net.layers[3].bias[:] = 0.0
    net.layers[3].bias[7] = 95.0  # exp overflows fp32 above 88.72
    dnn = _load(tmp_models, "float_ends_ovf.bin", net)
    x = F.synth_features(5, 20, seed=6, pad_from=None)
    try:
        probs = dnn.calculate(x)
    finally:
        dnn.delete()
    assert np.isnan(probs[:, 7]).all()
    rest = np.delete(probs, 7, axis=1)
    assert (rest == 0.0).all()


def test_subnormal_products_are_not_flushed(tmp_models):
    net = _ends_net()
    net.layers[0].weights[:] = (net.layers[0].weights * np.float32(1e-30)).astype(np.float32)
    net.layers[0].bias[:] = 0.0
    net.scale[:] = np.float32(1e-12)
    dnn = _load(tmp_models, "float_ends_sub.bin", net)
    x = F.synth_features(33, 20, seed=6, pad_from=None)
    try:
        cur = dnn.layer(-1, x)[1]
        lin, _ = dnn.layer(0, cur)
    finally:
        dnn.delete()
    ref = api.float_layer_ref(net.layers[0].weights, net.layers[0].bias, cur)
    assert FR.same_bits(lin, ref)
    tiny = np.abs(lin[lin != 0])
    assert tiny.size > lin.size // 2 and tiny.max() < 2.0 ** -126  # the sums ARE subnormal, and there
