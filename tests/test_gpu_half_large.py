"""The half net's large-batch kernel (fdnn_half_large.hip) under setLarge: the tiled kernel's BYTES, float64
under half_ref's bounds where chain() gives them, half_exact's EXACT sums at every ring phase, and which counters moved."""
import os

import numpy as np
import pytest

import float_ref as FR
import half_exact as HE
from fast_dnn_amd import api, formats as F
from test_gpu_half import _load, chain

pytestmark = pytest.mark.gpu

TINY = [20, 48, 48, 48, 131]


def _counts():
    return {**api.half_launches(), **api.half_small_launches(), **api.half_mid_launches(), **api.half_large_launches()}


def _moved(before):
    return {k: v - before[k] for k, v in _counts().items() if v != before[k]}


@pytest.fixture(scope="module")
def tiny(tmp_models):
    net = F.synth_net(TINY, seed=21, w0_std=0.05, w_std=0.3)
    dnn = _load(tmp_models, "half_large_tiny.bin", net)
    x = F.synth_features(513, 20, seed=4, pad_from=None)
    want = dnn.calculate(x)  # the tiled kernel's rows: computed once, shared, never written
    want.setflags(write=False)
    yield dnn, net, x, want
    dnn.delete()


def _both(dnn, net, x, what, large=1, mid=0, small=0):
    before = _counts()
    dnn.setSmall(small), dnn.setMid(mid), dnn.setLarge(large)
    try:
        got, _ = chain(dnn, net, x, what)  # every layer inside its float64 bound
        calc = dnn.calculate(x)
    finally:
        dnn.setSmall(0), dnn.setMid(0), dnn.setLarge(0)
    moved = _moved(before)
    assert moved.pop("input_step") == 2
    return got, calc, moved


def _all_of(kind):
    return {f"{kind}.sigmoid": 3, f"{kind}.exp": 1, f"{kind}.sigmoid.tap": 3, f"{kind}.exp.tap": 1}


@pytest.mark.parametrize("n,small,mid,large,takes", [(n, 0, 0, 1, "large") for n in (1, 127, 128, 129, 255, 256, 257, 513)] + [
    (128, 128, 4096, 1, "small"), (300, 0, 4096, 1, "mid"), (300, 0, 200, 250, "large"), (249, 0, 200, 250, "hgemm")])
def test_frames_and_rule(tiny, n, small, mid, large, takes):
    """One, two and three frame tiles of 256, both sides of a wave's 128-frame half; then small, mid, large, tiled in that order."""
    dnn, net, x, want = tiny
    got, calc, moved = _both(dnn, net, x[:n], f"{takes} n {n}", large, mid, small)
    assert FR.same_bits(got, want[:n]) and FR.same_bits(calc, want[:n]) and moved == _all_of(takes)


@pytest.mark.parametrize("hidden,out", [(16, 1), (16, 63), (16, 64), (16, 65), (16, 127), (16, 128), (16, 129), (16, 257), (144, 131)])
def test_widths(tmp_models, hidden, out):
    """Output widths around the 64-node partial and the 128-node tile; K_pad 32 and 160: half a stage, two and a half; n = 257."""
    net = F.synth_net([20, hidden, hidden, hidden, out], seed=7 + out, w0_std=0.05, w_std=0.3)
    dnn = _load(tmp_models, f"half_large_{hidden}_{out}.bin", net)
    x = F.synth_features(257, 20, seed=6, pad_from=None)
    try:
        want = dnn.calculate(x)
        got, calc, moved = _both(dnn, net, x, f"large {hidden} x {out}")
    finally:
        dnn.delete()
    assert FR.same_bits(got, want) and FR.same_bits(calc, want) and moved == _all_of("large")


@pytest.mark.parametrize("form,K", [("sigmoid", D) for D in (32, 64, 96, 128, 160, 192, 224, 2048, 2080, 4112, 1044)] + [("exp", H) for H in (96, 224, 352, 2048)])
def test_every_ring_phase(tmp_models, form, K):
    """The ring is three stages of 64 k.  K_pad = 32: one half stage; 64: one whole; 96 .. 224: two, three and four stages, whole
    and half last ones, so every stage count mod 3 with both last-stage lengths; 2048, 2080: 32 stages and 32 and a half; 4112
    (K_pad 4128): 64 and a half; 1044 (K_pad 1056): live -0 pad columns in the half stage; the exp form at one, three and five
    and a half stages and at 32.  n = 257.  z EQUALS the float64 sum; z and the stored bytes are the tiled kernel's."""
    (net, x), j = (HE.sig_case(K), 0) if form == "sigmoid" else (HE.exp_case(K), 3)
    x, l = x if j == 0 else x[3], net.layers[j]
    assert HE.premise(x, l.weights, l.bias) < HE.LIMIT
    z = HE.want(x, l.weights, l.bias)
    dnn = _load(tmp_models, f"half_large_{form}{K}.bin", net)
    os.remove(os.path.join(tmp_models, f"half_large_{form}{K}.bin"))  # the device holds the blob; the wide files are tens of megabytes
    try:
        tiled = dnn.layer(j, x)
        dnn.setLarge(1)
        before = _counts()
        lin, act = dnn.layer(j, x)
        assert _moved(before) == {f"large.{form}.tap": 1}
    finally:
        dnn.delete()
    assert FR.same_bits(lin, z), f"{int((lin != z).sum())} sums are not the exact ones"
    assert FR.same_bits(lin, tiled[0]) and FR.same_bits(act, tiled[1])


def test_rows_stay_in_their_rows(tmp_models):
    """The planted net of test_gpu_half_mid at 300 frames (a NaN row, an overflowing logit 7, all-zero rows): the clean rows keep
    their bytes, the whole result is the tiled kernel's; default chunk and chunks of 100 (every chunk large), both entry points."""
    import torch
    net = F.synth_net(TINY, seed=23, w0_std=0.05, w_std=0.3)
    net.layers[0].weights[:, 0] = 1.0
    for l in net.layers[1:3]:
        l.weights[:] = l.weights + np.float32(0.5)
        l.bias[:] = -18.0
    net.layers[3].weights[7, :], net.layers[3].bias[7] = 4.0, -90.0
    dnn = _load(tmp_models, "half_large_rows.bin", net)
    n, clean = 300, F.synth_features(300, 20, seed=4, pad_from=None)
    x = clean.copy()
    for first in (0, 100, 200):  # in every chunk of setChunk(100)
        x[first + 5, 3], x[first + 9, 0] = np.nan, 300.0
    x[64], x[299] = 0.0, 0.0
    dirty = np.isin(np.arange(n), [5, 9, 64, 105, 109, 205, 209, 299])
    side = torch.cuda.Stream()
    try:
        for chunk in (0, 100):
            chunks = 3 if chunk else 1
            dnn.setChunk(chunk)
            want, want_clean = dnn.calculate(x), dnn.calculate(clean)
            dnn.setLarge(1)
            before, got = _counts(), dnn.calculate(x)
            assert _moved(before) == {"large.sigmoid": 3 * chunks, "large.exp": chunks, "input_step": chunks}
            assert np.isnan(got[5]).all() and np.isnan(got[9, 7]) and (np.delete(got[9], 7) == 0.0).all()
            assert FR.same_bits(got[~dirty], want_clean[~dirty]) and FR.same_bits(got, want), chunk
            xd = torch.from_numpy(x).cuda()
            od = torch.zeros((n, 131), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            dnn.calculateDevice(xd.data_ptr(), n, od.data_ptr(), side.cuda_stream)
            torch.cuda.synchronize()
            assert FR.same_bits(od.cpu().numpy(), want), chunk
            dnn.setLarge(0)
    finally:
        dnn.delete()


def test_tail_chunk_of_one_frame(tiny):
    """4097 frames under the default chunk: 4096 + 1, both large."""
    dnn, net, _, _ = tiny
    x = F.synth_features(4097, 20, seed=9, pad_from=None)
    want, before = dnn.calculate(x), _counts()
    dnn.setLarge(1)
    try:
        got = dnn.calculate(x)
    finally:
        dnn.setLarge(0)
    assert _moved(before) == {"large.sigmoid": 6, "large.exp": 2, "input_step": 2} and FR.same_bits(got, want)


def test_lazy_sets_ride_along(tiny):
    """calculateLazySets at 300 frames, two segments: the hidden layers take the large kernel, the bytes stay."""
    dnn, net, x, want = tiny
    tables = ([0, 130, 300], [0, 5, 45], np.concatenate((np.arange(3, 8), np.arange(60, 100))).astype(np.int32))
    (want_p, want_i), before = dnn.calculateLazySets(x[:300], *tables), _counts()
    dnn.setLarge(1)
    try:
        got_p, got_i = dnn.calculateLazySets(x[:300], *tables)
    finally:
        dnn.setLarge(0)
    assert _moved(before) == {"large.sigmoid": 3, "input_step": 1} and FR.same_bits(got_p, want_p) and FR.same_bits(got_i, want_i)


@pytest.mark.parametrize("bad", [-1, 65537])
def test_arguments(tiny, bad):
    dnn, net, x, want = tiny
    dnn.setLarge(250)
    try:
        assert api.lib().fdnn_half_model_set_large(dnn.nativeHandle, bad) == api.FDNN_E_ARG
        before, _ = _counts(), (dnn.calculate(x[:249]), dnn.calculate(x[:250]))  # the setting is still 250: one tiled call, one large
        assert _moved(before) == {"hgemm.sigmoid": 3, "hgemm.exp": 1, "large.sigmoid": 3, "large.exp": 1, "input_step": 2}
    finally:
        dnn.setLarge(0)
