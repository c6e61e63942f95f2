"""The half net's four matrix kernels held to EXACT sums (tests/half_exact.py): on a fixed-point operand grid every order of
fp32 additions gives the float64 sum, so z must equal it bit for bit, at every K, in every form, and a lost, repeated or
skipped k-step, a stale ring slot or a neighbour's row or bias cannot pass (tests/test_half_exact_host.py holds the premise,
the sensitivity and that the tables reach every k-loop shape).  No tolerance appears in this file: the sums are compared by
FR.same_bits, the sigmoids by half_ref's bound and, like the probabilities, byte for byte across the kernels.  (What the
grid cannot see: a k-step that is -0 pad from end to end -- K = 4112 in K_pad 4128, K = 1072 in 1088 -- adds nothing.)

The Gaussian nets at the end reach the plain (non-tap) forms, which only calculate() runs, at multi-stage K."""
import os

import numpy as np
import pytest

import float_ref as FR
import half_exact as HE
import half_ref as HR
from fast_dnn_amd import api
from test_gpu_half import _load, chain

pytestmark = pytest.mark.gpu


def _counts():
    return {**api.half_launches(), **api.half_small_launches(), **api.half_mid_launches(), **api.half_set_launches()}


def _moved(before):
    return {k: v - before[k] for k, v in _counts().items() if v != before[k]}


def _open(tmp_models, name, net):
    dnn = _load(tmp_models, name, net)
    os.remove(os.path.join(tmp_models, name))  # the device holds the blob; the wide files are tens of megabytes
    return dnn


def _layer(dnn, j, x, kernel, small, mid, form):
    """dnn.layer(j, x) under one kernel's settings -> (lin, act); exactly one launch, of that kernel's tap form."""
    dnn.setSmall(small), dnn.setMid(mid)
    try:
        before = _counts()
        lin, act = dnn.layer(j, x)
        assert _moved(before) == {f"{kernel}.{form}.tap": 1}, (kernel, x.shape)
    finally:
        dnn.setSmall(0), dnn.setMid(0)
    return lin, act


def _dense(dnn, net, j, x, what, hidden_n=None):
    """Layer j on x[:n] under every kernel and frame count of HE.RUNS (hidden_n: one n per kernel): the sums are `want`, a
    sigmoid is inside half_ref's bound, and the stored halves or probabilities are byte-equal across the kernels."""
    l, last = net.layers[j], j + 1 == len(net.layers)
    form = "exp" if last else "sigmoid"
    z = HE.want(x, l.weights, l.bias)
    ref, exact = None, 0
    for kernel, small, mid, ns in reversed(HE.RUNS):  # the tiled kernel first: its n covers the others'
        for n in (hidden_n[kernel],) if hidden_n else ns:
            lin, act = _layer(dnn, j, x[:n], kernel, small, mid, form)
            assert FR.same_bits(lin, z[:n]), f"{what}: {kernel} n {n}: {int((lin != z[:n]).sum())} sums are not the exact ones"
            if not last:
                assert not HR.act_failures(act, lin).any(), f"{what}: {kernel} n {n}"
            if ref is None:
                ref = act
            assert FR.same_bits(act, ref[:n]), f"{what}: {kernel} n {n}: the stored bytes differ from the tiled kernel's"
            exact += 1
    return exact


@pytest.mark.parametrize("D", HE.SIG_D)
def test_sigmoid_forms_sweep_k(tmp_models, D):
    """Layer 0 of net(D, 80, 64): K = D walks every stage count and residue of the three dense kernels in the sigmoid form."""
    net, x = HE.sig_case(D)
    dnn = _open(tmp_models, f"half_exact_d{D}.bin", net)
    try:
        assert _dense(dnn, net, 0, x, f"D {D}") == 7
    finally:
        dnn.delete()


def _exp_and_set(tmp_models, H):
    net, xs = HE.exp_case(H)
    dnn = _open(tmp_models, f"half_exact_h{H}.bin", net)
    try:
        assert _dense(dnn, net, 3, xs[3], f"H {H} output") == 7
        last = net.layers[3]
        z = HE.want(xs[3], last.weights, last.bias)
        for length in HE.SET_LENS:
            nodes = np.sort(np.random.default_rng(H + length).choice(HE.EXP_O, length, replace=False)).astype(np.int32)
            for n in HE.SET_N:
                before = _counts()
                got = dnn.setLayer(xs[3][:n], nodes)[0]
                assert _moved(before) == {"set.score.tap": 1}, (H, length, n)
                assert FR.same_bits(got, z[:n][:, nodes]), f"H {H}: set of {length} at n {n}: not the exact sums"
        for j in (1, 2):  # sigmoid, K = H, H rows: many node tiles
            assert _dense(dnn, net, j, xs[j], f"H {H} layer {j}", HE.HIDDEN_N) == 3
    finally:
        dnn.delete()


@pytest.mark.parametrize("H", HE.EXP_H)
def test_exp_forms_and_set_kernel_sweep_k(tmp_models, H):
    """Layer 3 of net(20, H, 131) under the dense kernels and through setLayer, and the hidden layers 1 and 2 of the same net."""
    _exp_and_set(tmp_models, H)


def test_exp_forms_and_set_kernel_at_2048(tmp_models):
    """The bench width: 64 tiled steps, 16 mid stages, 8 small stages (24 to 48 tiles: the 9-tile ring goes round up to five
    times), the set kernel's whole resident image."""
    _exp_and_set(tmp_models, HE.EXP_H_WIDE)


# ------------------------------------------------------------------------------------------------------------ the plain forms
@pytest.fixture(scope="module", params=sorted(HE.PLAIN))
def plain(request, tmp_models):
    net, x = HE.plain_net(request.param), HE.plain_features(request.param)
    dnn = _open(tmp_models, f"half_exact_{request.param}.bin", net)
    want, _ = chain(dnn, net, x, f"{request.param} tiled n {HE.N_ROWS}")  # the tiled kernel, every layer inside its float64 bounds
    want.setflags(write=False)
    yield dnn, net, x, want
    dnn.delete()


@pytest.mark.parametrize("chunk", [0, 100])
@pytest.mark.parametrize("kernel,small,mid,n", [("small", 128, 0, 33), ("small", 128, 0, 128), ("mid", 0, 4096, 129), ("hgemm", 0, 0, 257)])
def test_plain_forms_at_multi_stage_k(plain, kernel, small, mid, n, chunk):
    """chain() (the tap forms, float64 bounds per layer) and calculate() (the plain forms) under each kernel: one set of bytes."""
    dnn, net, x, want = plain
    dnn.setChunk(chunk), dnn.setSmall(small), dnn.setMid(mid)
    try:
        before = _counts()
        got, _ = chain(dnn, net, x[:n], f"{kernel} n {n} chunk {chunk}")
        taps = _moved(before)
        before = _counts()
        calc = dnn.calculate(x[:n])
        plains = _moved(before)
    finally:
        dnn.setChunk(0), dnn.setSmall(0), dnn.setMid(0)
    chunks = -(-n // chunk) if chunk else 1
    assert taps == {f"{kernel}.sigmoid.tap": 3 * chunks, f"{kernel}.exp.tap": chunks, "input_step": 1}
    assert plains == {f"{kernel}.sigmoid": 3 * chunks, f"{kernel}.exp": chunks, "input_step": chunks}
    assert FR.same_bits(got, want[:n]) and FR.same_bits(calc, want[:n])


@pytest.mark.parametrize("mid", [0, 4096])
def test_lazy_sets_on_the_plain_nets(plain, mid):
    """calculateLazySets on two segments: the hidden layers run the plain forms (tiled or mid), the set step the resident-tile
    kernel; the blocks are setLayer's on the device's own last hidden rows."""
    dnn, net, x, want = plain
    O = net.layers[-1].out_dim
    h = dnn.layer(2, dnn.layer(1, dnn.layer(0, dnn.layer(-1, x)[1])[1])[1])[1]
    sets = [np.sort(np.random.default_rng(s).choice(O, length, replace=False)).astype(np.int32) for s, length in ((1, 33), (2, 70))]
    seg_rows = [0, 130, HE.N_ROWS]
    parts = [dnn.setLayer(h[a:b], s) for a, b, s in zip(seg_rows, seg_rows[1:], sets)]
    dnn.setMid(mid)
    try:
        before = _counts()
        probs, inactive = dnn.calculateLazySets(x, seg_rows, [0, 33, 103], np.concatenate(sets))
        moved = _moved(before)
    finally:
        dnn.setMid(0)
    assert moved == {("mid.sigmoid" if mid else "hgemm.sigmoid"): 3, "set.score": 1, "input_step": 1}
    assert FR.same_bits(probs, np.concatenate([p[1].ravel() for p in parts])) and FR.same_bits(inactive, np.concatenate([p[2] for p in parts]))
