"""Dense scoring with a top-k return through the model (fdnn_calculate_topk and its context, device, raw-frame and stream
forms): on every net the bytes are the contract's selection, stated in numpy (tests/topk_cases.py), on what the dense entry
point returns for the same frames; against the oracle every returned value is a 2e-6 probability of its node and no node left
out beats the smallest one returned by more than 4e-6."""
import numpy as np
import pytest

import lazy_lists_cases as LC
import topk_cases as TC
from fast_dnn_amd import api, formats as F
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu
KALDI = (list(range(-5, 6)), 39)
NETS = {"tiny": 33, "mid": 100, "lad/251": 33, "tail/ovf": 33, "full": 64, "n256/256/nosat": 33}  # net -> frames


@pytest.fixture(scope="module")
def fixtures(mid_model_path, sat_model_path, tiny_model_path, net_model_path):
    return {"mid": mid_model_path, "sat": sat_model_path, "tiny": tiny_model_path, "full": net_model_path}


@pytest.fixture(scope="module")
def nets(fixtures):
    """net -> (dnn, x, dense rows), loaded on first use and shared by the tests of this file."""
    cache = {}

    def get(net):
        if net not in cache:
            dnn = api.QuantizedDnn.loadFromFile(LC.model_path(net, fixtures))
            x = F.synth_features(NETS[net], LC.in_dim(net), seed=1200 + len(net))
            cache[net] = (dnn, x, dnn.calculate(x))
        return cache[net]

    yield get
    for dnn, _, _ in cache.values():
        dnn.delete()


def ks_of(O):
    return sorted({1, 32, min(O, 256)})


def same(got, want, k):
    nodes, probs = got
    return (nodes.shape == (want[0].shape[0], k) and nodes.dtype == np.int32 and probs.dtype == np.float32 and
            np.array_equal(nodes, want[0][:, :k]) and np.array_equal(probs.view(np.uint32), want[1][:, :k]))


@pytest.mark.parametrize("net", list(NETS))
def test_every_entry_point_returns_the_selection_of_the_dense_rows(nets, net):
    import torch

    dnn, x, dense = nets(net)
    n, O = dense.shape
    want = TC.select(dense, min(O, 256))
    if net == "tail/ovf":
        assert np.isnan(dense).any() or np.isinf(dense).any()  # the rows this net is here for
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutput(x)
    st = torch.cuda.Stream()
    dx = torch.from_numpy(x).cuda()
    for k in ks_of(O):
        assert same(dnn.calculateTopK(x, k), want, k), (net, k)
        assert same(ctx.calculateOutputTopK(k), want, k), (net, k)
        for form in ("ctx", "model"):
            dn = torch.full((n * k + 4,), -7, dtype=torch.int32, device="cuda")
            dp = torch.full((n * k + 4,), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            if form == "ctx":
                ctx.calculateOutputTopKDevice(k, dn.data_ptr(), dp.data_ptr(), st.cuda_stream)
            else:
                dnn.calculate_topk_device(dx.data_ptr(), n, k, dn.data_ptr(), dp.data_ptr(), st.cuda_stream)
            st.synchronize()
            assert (dn[n * k:] == -7).all() and (dp[n * k:] == -7.0).all()
            assert same((dn[:n * k].cpu().numpy().reshape(n, k), dp[:n * k].cpu().numpy().reshape(n, k)), want, k), (net, k, form)
    n31, p31 = dnn.calculateTopK(x, 31)
    n32, p32 = dnn.calculateTopK(x, 32)
    assert np.array_equal(n31, n32[:, :31]) and np.array_equal(p31.view(np.uint32), p32.view(np.uint32)[:, :31])
    ctx.delete()
    assert np.array_equal(dnn.calculate(x).view(np.uint32), dense.view(np.uint32))  # the dense entry point keeps its bytes


@pytest.mark.parametrize("net", list(NETS))
def test_raw_frames(nets, net):
    dnn, _, _ = nets(net)
    dnn.setSplice(*KALDI)
    try:
        raw = (np.random.default_rng(77).standard_normal((NETS[net], 39)) * 3).astype(np.float32)
        dense = dnn.calculateRaw(raw)
        O = dense.shape[1]
        want = TC.select(dense, min(O, 256))
        for k in ks_of(O):
            assert same(dnn.calculateTopKRaw(raw, k), want, k), (net, k)
    finally:
        dnn.setSplice([], 0)


def test_state_and_argument_errors(nets):
    dnn, x, _ = nets("tiny")
    ctx = dnn.getNewLazyContext(x.shape[0])
    with pytest.raises(api.FdnnError) as e:
        ctx.calculateOutputTopK(5)  # before the hidden layers
    assert e.value.code == api.FDNN_E_STATE
    ctx.delete()
    for k in (0, 101, 257):
        with pytest.raises(api.FdnnError) as e:
            dnn.calculateTopK(x, k)
        assert e.value.code == api.FDNN_E_ARG


def test_a_call_of_two_chunks_equals_two_calls(nets):
    dnn, _, _ = nets("mid")
    n = 20480 + 300
    for chained in (True, False):
        assert len(api.frame_chunks(n, chained)) >= 2
    x = F.synth_features(n, 432, seed=1300)
    k = 32
    nodes, probs = dnn.calculateTopK(x, k)
    cut = api.frame_chunks(n, True)[1][0]
    a, b = dnn.calculateTopK(x[:cut], k), dnn.calculateTopK(x[cut:], k)
    assert np.array_equal(nodes, np.concatenate([a[0], b[0]])) and np.array_equal(probs.view(np.uint32), np.concatenate([a[1], b[1]]).view(np.uint32))
    rows = [0, 1, cut - 1, cut, n - 1]  # ... which are the selection of the dense rows
    want = TC.select(dnn.calculate(x[rows]), k)
    assert np.array_equal(nodes[rows], want[0]) and np.array_equal(probs[rows].view(np.uint32), want[1])


def test_raw_and_device_calls_of_two_chunks_equal_two_calls(nets):
    """fdnn_calculate_topk_raw and fdnn_calculate_topk_device at the smallest n that api.frame_chunks cuts in two, on the tiny
    net: the second chunk's rows are spliced from row `cut` on (raw) or read at d_x + cut * D (device), and its pairs land at
    cut * k of the caller's arrays -- the bytes of the same rows scored as two calls."""
    import torch

    from fast_dnn_amd import convert as CV

    dnn, _, _ = nets("tiny")
    n, k = 20480 + 1, 32
    for chained in (True, False):
        assert len(api.frame_chunks(n, chained)) == 2 and len(api.frame_chunks(n - 1, chained)) == 1
    cut = api.frame_chunks(n, True)[1][0]

    def in_two_calls(rows):
        a, b = dnn.calculateTopK(rows[:cut], k), dnn.calculateTopK(rows[cut:], k)
        return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]).view(np.uint32)

    raw = (np.random.default_rng(79).standard_normal((n, 39)) * 3).astype(np.float32)
    dnn.setSplice(*KALDI)
    try:
        got = dnn.calculateTopKRaw(raw, k)
    finally:
        dnn.setSplice([], 0)
    assert same(got, in_two_calls(CV.splice_frames(raw, KALDI[0], 432)), k)
    x = F.synth_features(n, 432, seed=1301)
    dx = torch.from_numpy(x).cuda()
    dn = torch.full((n * k + 4,), -7, dtype=torch.int32, device="cuda")
    dp = torch.full((n * k + 4,), -7.0, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    dnn.calculate_topk_device(dx.data_ptr(), n, k, dn.data_ptr(), dp.data_ptr(), st.cuda_stream)
    st.synchronize()
    assert (dn[n * k:] == -7).all() and (dp[n * k:] == -7.0).all()
    assert same((dn[:n * k].cpu().numpy().reshape(n, k), dp[:n * k].cpu().numpy().reshape(n, k)), in_two_calls(x), k)


def test_a_hidden_only_stream_push(nets):
    dnn, _, _ = nets("mid")
    dnn.setSplice(*KALDI)
    try:
        raw = (np.random.default_rng(78).standard_normal((90, 39)) * 3).astype(np.float32)
        dense = dnn.calculateRaw(raw)
        st = dnn.newStream(64)
        got, done = [], 0
        for i in (0, 64):
            ctx = st.pushHidden(raw[i:i + 64], end=i + 64 >= len(raw))
            rows = ctx.inputVectorCount
            got.append((ctx.calculateOutputTopK(32), done, rows))
            done += rows
        st.close()
        assert done == len(raw)
        for res, first, rows in got:
            assert rows > 0 and same(res, TC.select(dense[first:first + rows], 32), 32)
    finally:
        dnn.setSplice([], 0)


@pytest.mark.parametrize("net", ["tiny", "mid", "full"])
def test_against_the_oracle_on_every_row(nets, fixtures, net):
    dnn, x, _ = nets(net)
    orc = Oracle(LC.model_path(net, fixtures))
    p = orc.output_mt(orc.hidden_acts_mt(x))
    assert np.isfinite(p).all()
    n, O = p.shape
    for k in ks_of(O):
        nodes, probs = dnn.calculateTopK(x, k)
        near = np.abs(probs.astype(np.float64) - np.take_along_axis(p, nodes.astype(np.int64), axis=1).astype(np.float64))
        print(f"{net} k={k}: max |value - oracle| = {near.max():.3e}")
        assert near.max() <= LC.TIGHT
        left = p.astype(np.float64).copy()
        np.put_along_axis(left, nodes.astype(np.int64), -np.inf, axis=1)
        if k < O:
            over = left.max(1) - probs[:, -1].astype(np.float64)
            print(f"{net} k={k}: max (unreturned oracle - smallest returned) = {over.max():.3e}")
            assert (over <= 4e-6).all()
        for f in range(n):
            assert len(set(nodes[f].tolist())) == k
