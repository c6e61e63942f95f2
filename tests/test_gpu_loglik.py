"""Decoder scores through the model (fdnn_calculate_loglik and its context, device, raw-frame and stream forms), on the nets
tests/test_gpu_pool.py uses: on every net every entry point's bytes are the contract's score (api.loglik_ref, held to numpy
and the one logarithm by tests/test_loglik_host.py) of what the dense entry point returns for the same frames -- the dense
pass is untouched, so the composition is exact -- for fp32 and fp16 handles, with and without a floor."""
import numpy as np
import pytest

import lazy_lists_cases as LC
import loglik_cases as LL
from fast_dnn_amd import api, formats as F

pytestmark = pytest.mark.gpu
KALDI = (list(range(-5, 6)), 39)
NETS = {"tiny": 33, "mid": 100, "lad/251": 33, "tail/ovf": 33, "full": 64, "n256/256/nosat": 33}  # net -> frames
HANDLES = ((-np.inf, api.LOGLIK_F32), (-20.0, api.LOGLIK_F32), (-np.inf, api.LOGLIK_F16), (-20.0, api.LOGLIK_F16))


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
            x = F.synth_features(NETS[net], LC.in_dim(net), seed=1800 + len(net))
            cache[net] = (dnn, x, dnn.calculate(x))
        return cache[net]

    yield get
    for dnn, _, _ in cache.values():
        dnn.delete()


def device_scores(torch, d_out, n, O, t):
    got = d_out.cpu().numpy()
    assert (got[n * O:] == -7).all()
    return got[:n * O].view(np.float16 if t == api.LOGLIK_F16 else np.float32).reshape(n, O)


@pytest.mark.parametrize("net", list(NETS))
def test_every_entry_point_returns_the_scores_of_the_dense_rows(nets, net):
    import torch

    dnn, x, dense = nets(net)
    n, O = dense.shape
    if net == "tail/ovf":
        assert np.isnan(dense).any() or np.isinf(dense).any()  # the rows this net is here for
    lp = LL.priors(O)
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutput(x)
    st = torch.cuda.Stream()
    dx = torch.from_numpy(x).cuda()
    for floor, t in HANDLES:
        ll = api.Loglik(lp, floor, t)
        want = api.loglik_ref(dense, lp, floor, t)
        got = dnn.calculateLoglik(x, ll)
        assert got.shape == (n, O) and got.dtype == want.dtype and LL.same_bytes(got, want), (net, floor, t)
        assert LL.same_bytes(ctx.calculateOutputLoglik(ll), want), (net, floor, t)
        if np.isfinite(floor):
            assert not np.isneginf(got).any()  # with a finite floor no -inf leaves the device
        for form in ("ctx", "model"):
            dq = torch.full((n * O + 4,), -7, dtype=torch.int16 if t == api.LOGLIK_F16 else torch.int32, device="cuda")
            torch.cuda.synchronize()
            if form == "ctx":
                ctx.calculateOutputLoglikDevice(ll, dq.data_ptr(), st.cuda_stream)
            else:
                dnn.calculate_loglik_device(dx.data_ptr(), n, ll, dq.data_ptr(), st.cuda_stream)
            st.synchronize()
            assert LL.same_bytes(device_scores(torch, dq, n, O, t), want), (net, floor, t, form)
        ll.delete()
    ctx.delete()
    assert np.array_equal(dnn.calculate(x).view(np.uint32), dense.view(np.uint32))  # the dense entry point keeps its bytes


@pytest.mark.parametrize("net", list(NETS))
def test_raw_frames(nets, net):
    dnn, _, _ = nets(net)
    dnn.setSplice(*KALDI)
    try:
        raw = (np.random.default_rng(97).standard_normal((NETS[net], 39)) * 3).astype(np.float32)
        dense = dnn.calculateRaw(raw)
        lp = LL.priors(dense.shape[1])
        for floor, t in ((-20.0, api.LOGLIK_F16), (-np.inf, api.LOGLIK_F32)):
            ll = api.Loglik(lp, floor, t)
            assert LL.same_bytes(dnn.calculateLoglikRaw(raw, ll), api.loglik_ref(dense, lp, floor, t)), (net, t)
            ll.delete()
    finally:
        dnn.setSplice([], 0)


def test_state_and_argument_errors(nets):
    import torch

    dnn, x, dense = nets("tiny")
    n, O = dense.shape
    ll = api.Loglik(LL.priors(O), -20.0, api.LOGLIK_F16)
    ctx = dnn.getNewLazyContext(n)
    with pytest.raises(api.FdnnError) as e:
        ctx.calculateOutputLoglik(ll)  # before the hidden layers
    assert e.value.code == api.FDNN_E_STATE
    ctx.calculateUntilOutput(x)
    narrow = api.Loglik(np.zeros(O - 1, np.float32))
    wide = api.Loglik(np.zeros(O + 1, np.float32), -1.0, api.LOGLIK_F16)
    before = api.loglik_launches()
    dq = torch.full((n * O,), -7, dtype=torch.int32, device="cuda")
    for bad in (narrow, wide):  # width mismatch: before anything is launched
        for call in (lambda: dnn.calculateLoglik(x, bad), lambda: ctx.calculateOutputLoglik(bad),
                     lambda: ctx.calculateOutputLoglikDevice(bad, dq.data_ptr()), lambda: dnn.calculate_loglik_device(0, 4, bad, dq.data_ptr())):
            with pytest.raises(api.FdnnError) as e:
                call()
            assert e.value.code == api.FDNN_E_ARG
    L = api.lib()
    f32p = api.C.POINTER(api.C.c_float)
    xp = x.ctypes.data_as(f32p)
    out = np.empty((n, O), np.float16)
    op = api.C.c_void_p(out.ctypes.data)
    assert L.fdnn_calculate_loglik(dnn.nativeDnnHandle, xp, n, x.shape[1], None, op) == api.FDNN_E_ARG          # null handle
    assert L.fdnn_calculate_loglik(dnn.nativeDnnHandle, None, n, x.shape[1], ll.handle, op) == api.FDNN_E_ARG   # null frames
    assert L.fdnn_calculate_loglik(dnn.nativeDnnHandle, xp, n, x.shape[1], ll.handle, None) == api.FDNN_E_ARG   # null result
    assert L.fdnn_calculate_loglik(dnn.nativeDnnHandle, xp, n, x.shape[1] - 1, ll.handle, op) == api.FDNN_E_ARG  # input width
    assert L.fdnn_calculate_loglik(None, xp, n, x.shape[1], ll.handle, op) == api.FDNN_E_ARG
    assert L.fdnn_ctx_output_loglik(ctx.handle, ll.handle, None) == api.FDNN_E_ARG
    assert L.fdnn_ctx_output_loglik(None, ll.handle, op) == api.FDNN_E_ARG
    assert L.fdnn_ctx_output_loglik_device(ctx.handle, ll.handle, None, None) == api.FDNN_E_ARG
    assert L.fdnn_calculate_loglik_device(dnn.nativeDnnHandle, None, 4, ll.handle, dq.data_ptr(), None) == api.FDNN_E_ARG
    assert L.fdnn_calculate_loglik_device(dnn.nativeDnnHandle, dq.data_ptr() + 4, 4, ll.handle, dq.data_ptr(), None) == api.FDNN_E_ARG  # frames off 16 bytes
    with pytest.raises(api.FdnnError) as e:
        dnn.calculateLoglikRaw(np.zeros((4, 39), np.float32), ll)  # no splice spec
    assert e.value.code == api.FDNN_E_STATE
    torch.cuda.synchronize()
    assert api.loglik_launches() == before and (dq == -7).all()
    assert dnn.calculateLoglik(x[:0], ll).shape == (0, O)  # n == 0: nothing to do
    for h in (ll, narrow, wide):
        h.delete()
    ctx.delete()


def test_a_call_of_two_chunks_equals_two_calls(nets):
    dnn, _, dense = nets("mid")
    n = 20480 + 300
    for chained in (True, False):
        assert len(api.frame_chunks(n, chained)) >= 2
    x = F.synth_features(n, 432, seed=1900)
    lp = LL.priors(dense.shape[1])
    ll = api.Loglik(lp, -20.0, api.LOGLIK_F16)
    got = dnn.calculateLoglik(x, ll)
    cut = api.frame_chunks(n, True)[1][0]
    a, b = dnn.calculateLoglik(x[:cut], ll), dnn.calculateLoglik(x[cut:], ll)
    assert LL.same_bytes(got, np.concatenate([a, b]))
    rows = [0, 1, cut - 1, cut, n - 1]  # ... which are the scores of the dense rows
    assert LL.same_bytes(got[rows], api.loglik_ref(dnn.calculate(x[rows]), lp, -20.0, api.LOGLIK_F16))
    ll.delete()


@pytest.mark.parametrize("t", LL.TYPES)
def test_a_device_call_of_two_chunks_equals_two_calls(nets, t):
    """The second chunk's scores start at cut x O elements of the caller's buffer, whatever the element's size."""
    import torch

    dnn, _, dense = nets("tiny")
    n, O = 20480 + 1, dense.shape[1]
    for chained in (True, False):
        assert len(api.frame_chunks(n, chained)) == 2
    cut = api.frame_chunks(n, True)[1][0]
    lp = LL.priors(O)
    ll = api.Loglik(lp, -np.inf, t)
    x = F.synth_features(n, 432, seed=1901)
    dx = torch.from_numpy(x).cuda()
    dq = torch.full((n * O + 4,), -7, dtype=torch.int16 if t == api.LOGLIK_F16 else torch.int32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    dnn.calculate_loglik_device(dx.data_ptr(), n, ll, dq.data_ptr(), st.cuda_stream)
    st.synchronize()
    want = np.concatenate([dnn.calculateLoglik(x[:cut], ll), dnn.calculateLoglik(x[cut:], ll)])
    assert LL.same_bytes(device_scores(torch, dq, n, O, t), want)
    ll.delete()


def test_a_hidden_only_stream_push(nets):
    dnn, _, dense0 = nets("mid")
    lp = LL.priors(dense0.shape[1])
    ll = api.Loglik(lp, -20.0, api.LOGLIK_F16)
    dnn.setSplice(*KALDI)
    try:
        raw = (np.random.default_rng(98).standard_normal((90, 39)) * 3).astype(np.float32)
        dense = dnn.calculateRaw(raw)
        st = dnn.newStream(64)
        got, done = [], 0
        for i in (0, 64):
            ctx = st.pushHidden(raw[i:i + 64], end=i + 64 >= len(raw))
            rows = ctx.inputVectorCount
            got.append((ctx.calculateOutputLoglik(ll), done, rows))
            done += rows
        st.close()
        assert done == len(raw)
        for res, first, rows in got:
            assert rows > 0 and LL.same_bytes(res, api.loglik_ref(dense[first:first + rows], lp, -20.0, api.LOGLIK_F16))
    finally:
        dnn.setSplice([], 0)
        ll.delete()


def test_the_scores_are_the_logarithm_of_the_oracles_probabilities(nets, fixtures):
    """Against something independent of the library's logarithm: float64 log of the dense rows minus the priors, within
    kLnMaxUlp ulps of ln plus the subtraction's half ulp (fp32), and that rounded once more to fp16 (half an fp16 ulp)."""
    dnn, x, dense = nets("mid")
    lp = LL.priors(dense.shape[1])
    ll = api.Loglik(lp, -np.inf, api.LOGLIK_F32)
    s = dnn.calculateLoglik(x, ll)
    ll.delete()
    h = api.Loglik(lp, -np.inf, api.LOGLIK_F16)
    s16 = dnn.calculateLoglik(x, h)
    h.delete()
    LL.assert_log_of_rows(dense, lp, s, s16)
