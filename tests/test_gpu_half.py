"""The half-precision net on the device (fdnn_half.hip; contract: csrc/fdnn_half.hpp) against float64 under the derived
bounds of tests/half_ref.py, every layer judged alone on the fp16 operands the device used, and against its own invariance.

  1  sums: |z - z64| <= g'(K + 1) (sum |x w| + |b|) + K 2^-126, u' = 2^-23 -- one WHOLE ulp per addition, any order: products
     of two halves are exact in fp32, and the order (or a truncating alignment) inside one MFMA is not documented
  2  hidden activation: float_ref.sigmoid_bound(z) + 2^-11 sigma + 2^-25       3  soft-max: softmax_ref.check on the tap logits
  4  the input step is its restatement bit for bit: RN16(RN32(RN32(x + shift) * scale))
  5  a row's bytes do not depend on the batch, the position, the chunk or the entry point
"""
import os

import numpy as np
import pytest

import float_ref as FR
import half_ref as HR
import softmax_ref as SR
from fast_dnn_amd import api, formats as F

pytestmark = pytest.mark.gpu

TIGHT = 2e-6  # the suite's absolute bar on a probability


def _load(tmp_models, name, net):
    p = os.path.join(tmp_models, name)
    F.write_model_bin(p, net)
    return api.HalfDnn.loadFromFile(p, device=0)


def chain(dnn, net, x, what, soft_max=True):
    """The net layer by layer through fdnn_debug_half_layer, each layer held to items 1-4 -> (probabilities, logits)."""
    lin, cur = dnn.layer(-1, x)
    t = (x + net.shift[None, :]).astype(np.float32)
    assert FR.same_bits(lin, t) and FR.same_bits(cur, HR.halves((t * net.scale[None, :]).astype(np.float32))), f"{what}: input step"
    last = len(net.layers) - 1
    for j, l in enumerate(net.layers):
        lin, act = dnn.layer(j, cur)
        bad = HR.lin_failures(lin, cur, HR.halves(l.weights), l.bias)
        assert not bad.any(), f"{what}: layer {j}: {int(bad.sum())} sums outside the float64 bound"
        if j < last:
            bad = HR.act_failures(act, lin)
            assert not bad.any(), f"{what}: layer {j}: {int(bad.sum())} activations outside the bound"
        elif soft_max:
            SR.check(act, lin, SR.rows_pad_of(l.out_dim), f"{what}: soft-max", c_e=FR.C_E)
            assert np.abs(act.astype(np.float64) - SR.softmax64(lin)).max() <= TIGHT, what
        cur = act
    return cur, lin


@pytest.fixture(scope="module")
def tiny(tmp_models):
    net = F.synth_net([20, 48, 48, 48, 131], seed=21, w0_std=0.05, w_std=0.3)
    dnn = _load(tmp_models, "half_tiny.bin", net)
    x = F.synth_features(300, 20, seed=4, pad_from=None)
    want, _ = chain(dnn, net, x, "tiny n 300")  # computed once, shared, never written
    want.setflags(write=False)
    yield dnn, net, x, want
    dnn.delete()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 300])
def test_tiny_every_layer(tiny, n):
    dnn, net, x, want = tiny
    before = api.half_launches()
    got, _ = chain(dnn, net, x[:n], f"tiny n {n}")
    assert FR.same_bits(got, want[:n])  # item 5: the batch
    assert FR.same_bits(dnn.calculate(x[:n]), want[:n])  # the composition of the per-layer calls
    d = {k: v - before[k] for k, v in api.half_launches().items()}
    # the chain runs the tap forms (3 hidden + 1 output), calculate the plain ones; one input step each
    assert d == {"hgemm.sigmoid": 3, "hgemm.exp": 1, "hgemm.sigmoid.tap": 3, "hgemm.exp.tap": 1, "input_step": 2}


def test_rows_do_not_depend_on_batch_position_chunk_or_entry_point(tiny):
    import torch

    dnn, net, x, want = tiny
    for n, first in ((1, 0), (1, 299), (33, 100), (257, 43), (300, 0)):
        assert FR.same_bits(dnn.calculate(x[first:first + n]), want[first:first + n]), (n, first)
    perm = np.random.default_rng(1).permutation(300)
    assert FR.same_bits(dnn.calculate(x[perm]), want[perm])
    xd = torch.from_numpy(x).cuda()
    side = torch.cuda.Stream()
    try:
        for chunk in (100, 256, 0):  # not a multiple of the frame tile, the tile, the default
            dnn.setChunk(chunk)
            assert FR.same_bits(dnn.calculate(x), want), chunk
            for stream in (0, side.cuda_stream):
                od = torch.zeros((300, 131), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                dnn.calculateDevice(xd.data_ptr(), 300, od.data_ptr(), stream)
                torch.cuda.synchronize()
                assert FR.same_bits(od.cpu().numpy(), want), (chunk, stream)
            act = dnn.layer(3, dnn.layer(2, dnn.layer(1, dnn.layer(0, dnn.layer(-1, x)[1])[1])[1])[1])[1]
            assert FR.same_bits(act, want), chunk
    finally:
        dnn.setChunk(0)


def test_long_k_layer(tmp_models):
    """K = 1040: 32 k-steps and half a step.  Every |x w| term is at least 0.5625 and the bound at most g'(1041) 1043 = 0.13,
    under half a term: a lost, repeated or skipped term, or the neighbour's bias (2 away), leaves the bound."""
    x, w, b = HR.long_k_case()
    bound, t_min = HR.long_k_margin(x, w, b)
    assert bound < 0.5 * t_min and t_min >= 0.5625
    K = HR.K_LONG
    zeros = F.FloatLayerSpec(np.zeros((K, K), np.float32), np.zeros(K, np.float32))
    net = F.FloatNet([F.FloatLayerSpec(np.zeros((K, 20), np.float32), np.zeros(K, np.float32)), zeros, zeros, F.FloatLayerSpec(w, b)],
                     np.zeros(20, np.float32), np.ones(20, np.float32))
    dnn = _load(tmp_models, "half_longk.bin", net)
    try:
        lin, _ = dnn.layer(3, x)
    finally:
        dnn.delete()
    bad = HR.lin_failures(lin, x, w, b)
    assert not bad.any(), f"{int(bad.sum())} sums outside the float64 bound"


@pytest.mark.parametrize("hidden,out", [(16, 1), (16, 63), (16, 64), (16, 65), (16, 255), (16, 256), (16, 257), (144, 131)])
def test_widths(tmp_models, hidden, out):
    """Output widths around the 64-node partial and the 256-node tile; hidden widths 16 and 144 (no multiple of the node tile)."""
    net = F.synth_net([20, hidden, hidden, hidden, out], seed=7 + out, w0_std=0.05, w_std=0.3)
    dnn = _load(tmp_models, f"half_{hidden}_{out}.bin", net)
    x = F.synth_features(70, 20, seed=6, pad_from=None)
    try:
        want, _ = chain(dnn, net, x, f"{hidden} x {out}")
        got = dnn.calculate(x)
    finally:
        dnn.delete()
    assert FR.same_bits(got, want)


def test_edges(tiny, tmp_models):
    """A NaN in x stays in its row; the sigmoid's ends come from the arithmetic; an overflowing logit is NaN, the rest of its row 0."""
    dnn, net, x, want = tiny
    xn = x[:130].copy()
    xn[77, 5] = np.nan
    got = dnn.calculate(xn)
    keep = np.arange(130) != 77
    assert np.isnan(got[77]).all() and FR.same_bits(got[keep], want[:130][keep])
    net = F.synth_net([20, 48, 48, 48, 131], seed=23)
    net.layers[1].bias[0::2], net.layers[1].bias[1::2] = 120.0, -120.0
    net.layers[3].weights[:] = (net.layers[3].weights * np.float32(0.01)).astype(np.float32)
    net.layers[3].bias[:] = 0.0
    net.layers[3].bias[7] = 95.0  # exp overflows fp32 above 88.72
    ends = _load(tmp_models, "half_ends.bin", net)
    try:
        lin, act = ends.layer(1, ends.layer(0, ends.layer(-1, x[:33])[1])[1])
        probs = ends.calculate(x[:33])
    finally:
        ends.delete()
    assert (lin[:, 0::2] >= 104).all() and (lin[:, 1::2] <= -89).all()
    assert (act[:, 0::2] == 1.0).all() and (act[:, 1::2] == 0.0).all() and not np.signbit(act).any()
    assert np.isnan(probs[:, 7]).all() and (np.delete(probs, 7, axis=1) == 0.0).all()


def test_subnormal_halves_count(tmp_models):
    """Weights that are SUBNORMAL in fp16 (m 2^-24, m = 1 .. 1023) against activations of 1.0: the sums are the float64 values
    (within bound 1; they are exact here) and not 0 -- gfx950's fp16 MFMA does not flush subnormal operands."""
    net = F.synth_net([20, 48, 48, 48, 131], seed=23)
    m = np.random.default_rng(2).integers(1, 1024, (48, 48))
    net.layers[1].weights[:] = (m * 2.0 ** -24).astype(np.float32)
    net.layers[1].bias[:] = 0.0
    dnn = _load(tmp_models, "half_sub.bin", net)
    ones = np.ones((33, 48), np.float32)
    try:
        lin, _ = dnn.layer(1, ones)
    finally:
        dnn.delete()
    w = HR.halves(net.layers[1].weights)
    assert np.array_equal(w, net.layers[1].weights) and (w < 2.0 ** -14).all()
    print("subnormal sums: device", lin[0, :4], "float64", FR.lin64(ones, w, net.layers[1].bias)[0, :4])
    assert not HR.lin_failures(lin, ones, w, net.layers[1].bias).any() and (lin > 0).all()


def test_argument_errors_and_load_rejection(tiny, tmp_models):
    dnn = tiny[0]
    L, h = api.lib(), dnn.nativeHandle
    assert (dnn.inputDimension(), dnn.outputDimension(), dnn.layerCount(), dnn.layerDimension(3), dnn.layerDimension(4)) == (20, 131, 4, 131, -1)
    assert L.fdnn_debug_half_layer(h, 4, None, 1, None, None) == api.FDNN_E_ARG  # layer index out of range
    assert L.fdnn_debug_half_layer(h, 0, None, 1, None, None) == api.FDNN_E_ARG  # null buffer
    assert L.fdnn_half_calculate(h, None, 1, 20, None) == api.FDNN_E_ARG
    assert L.fdnn_half_calculate_device(h, None, 1, None, None) == api.FDNN_E_ARG
    one = np.zeros((1, 19), np.float32)
    assert L.fdnn_half_calculate(h, one.ctypes.data_as(api._c_f32p), 1, 19, one.ctypes.data_as(api._c_f32p)) == api.FDNN_E_ARG  # wrong dim
    assert dnn.layerMicros(1, np.full((130, 48), 0.5, np.float32), reps=2) > 0.0
    net = F.synth_net([20, 48, 48, 48, 131], seed=23)
    net.layers[2].weights[5, 9] = 65519.0  # the largest fp32 that still rounds to a finite half (65504)
    _load(tmp_models, "half_big.bin", net).delete()
    net.layers[2].weights[5, 9] = -65520.0
    with pytest.raises(api.FdnnError) as e:
        _load(tmp_models, "half_inf.bin", net)
    assert e.value.code == api.FDNN_E_FORMAT and "layer 2, node 5" in str(e.value)
