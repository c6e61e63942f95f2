"""Class posteriors through the model (fdnn_calculate_pool and its context, device, raw-frame and stream forms), on the nets
tests/test_gpu_topk.py uses: on every net the bytes are the contract's sum (api.pool_ref, held to numpy and float64 by
tests/test_pool_host.py) of what the dense entry point returns for the same frames; against the oracle's probabilities summed
in float64 every class sum stays within the project's 2e-6 per probability plus the derived bound of the additions."""
import numpy as np
import pytest

import lazy_lists_cases as LC
import pool_cases as PC
from fast_dnn_amd import api, formats as F
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu
KALDI = (list(range(-5, 6)), 39)
NETS = {"tiny": 33, "mid": 100, "lad/251": 33, "tail/ovf": 33, "full": 64, "n256/256/nosat": 33}  # net -> frames
MAPS = ("interleaved", "sizes", "quarter_out", "one")


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
            x = F.synth_features(NETS[net], LC.in_dim(net), seed=1500 + len(net))
            cache[net] = (dnn, x, dnn.calculate(x))
        return cache[net]

    yield get
    for dnn, _, _ in cache.values():
        dnn.delete()


@pytest.mark.parametrize("net", list(NETS))
def test_every_entry_point_returns_the_pool_of_the_dense_rows(nets, net):
    import torch

    dnn, x, dense = nets(net)
    n, O = dense.shape
    if net == "tail/ovf":
        assert np.isnan(dense).any() or np.isinf(dense).any()  # the rows this net is here for
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutput(x)
    st = torch.cuda.Stream()
    dx = torch.from_numpy(x).cuda()
    for mk in MAPS:
        co, C = PC.map_of(mk, O)
        pool = api.ClassPool(co, C)
        want = api.pool_ref(dense, co, C)
        got = dnn.calculatePool(x, pool)
        assert got.shape == (n, C) and got.dtype == np.float32 and PC.same_bytes(got, want), (net, mk)
        assert PC.same_bytes(ctx.calculateOutputPool(pool), want), (net, mk)
        for form in ("ctx", "model"):
            dq = torch.full((n * C + 4,), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            if form == "ctx":
                ctx.calculateOutputPoolDevice(pool, dq.data_ptr(), st.cuda_stream)
            else:
                dnn.calculate_pool_device(dx.data_ptr(), n, pool, dq.data_ptr(), st.cuda_stream)
            st.synchronize()
            assert (dq[n * C:] == -7.0).all()
            assert PC.same_bytes(dq[:n * C].cpu().numpy().reshape(n, C), want), (net, mk, form)
        pool.delete()
    ctx.delete()
    assert np.array_equal(dnn.calculate(x).view(np.uint32), dense.view(np.uint32))  # the dense entry point keeps its bytes


@pytest.mark.parametrize("net", list(NETS))
def test_raw_frames(nets, net):
    dnn, _, _ = nets(net)
    dnn.setSplice(*KALDI)
    try:
        raw = (np.random.default_rng(87).standard_normal((NETS[net], 39)) * 3).astype(np.float32)
        dense = dnn.calculateRaw(raw)
        co, C = PC.map_of("interleaved", dense.shape[1])
        pool = api.ClassPool(co, C)
        assert PC.same_bytes(dnn.calculatePoolRaw(raw, pool), api.pool_ref(dense, co, C)), net
        pool.delete()
    finally:
        dnn.setSplice([], 0)


def test_state_and_argument_errors(nets):
    import torch

    dnn, x, dense = nets("tiny")
    O = dense.shape[1]
    co, C = PC.map_of("interleaved", O)
    pool = api.ClassPool(co, C)
    ctx = dnn.getNewLazyContext(x.shape[0])
    with pytest.raises(api.FdnnError) as e:
        ctx.calculateOutputPool(pool)  # before the hidden layers
    assert e.value.code == api.FDNN_E_STATE
    ctx.calculateUntilOutput(x)
    narrow = api.ClassPool(np.zeros(O - 1, np.int32), 1)
    wide = api.ClassPool(np.zeros(O + 1, np.int32), 1)
    before = api.pool_launches()
    dq = torch.full((x.shape[0] * C,), -7.0, dtype=torch.float32, device="cuda")
    for bad in (narrow, wide):  # width mismatch: before anything is launched
        for call in (lambda: dnn.calculatePool(x, bad), lambda: ctx.calculateOutputPool(bad),
                     lambda: ctx.calculateOutputPoolDevice(bad, dq.data_ptr()), lambda: dnn.calculate_pool_device(0, 4, bad, dq.data_ptr())):
            with pytest.raises(api.FdnnError) as e:
                call()
            assert e.value.code == api.FDNN_E_ARG
    L = api.lib()
    f32p = api.C.POINTER(api.C.c_float)
    xp = x.ctypes.data_as(f32p)
    out = np.empty((x.shape[0], C), np.float32)
    op = out.ctypes.data_as(f32p)
    assert L.fdnn_calculate_pool(dnn.nativeDnnHandle, xp, x.shape[0], x.shape[1], None, op) == api.FDNN_E_ARG       # null pool
    assert L.fdnn_calculate_pool(dnn.nativeDnnHandle, None, x.shape[0], x.shape[1], pool.handle, op) == api.FDNN_E_ARG  # null frames
    assert L.fdnn_calculate_pool(dnn.nativeDnnHandle, xp, x.shape[0], x.shape[1], pool.handle, None) == api.FDNN_E_ARG  # null result
    assert L.fdnn_calculate_pool(None, xp, x.shape[0], x.shape[1], pool.handle, op) == api.FDNN_E_ARG
    assert L.fdnn_ctx_output_pool(ctx.handle, pool.handle, None) == api.FDNN_E_ARG
    assert L.fdnn_ctx_output_pool(None, pool.handle, op) == api.FDNN_E_ARG
    assert L.fdnn_ctx_output_pool_device(ctx.handle, pool.handle, None, None) == api.FDNN_E_ARG
    assert L.fdnn_calculate_pool_device(dnn.nativeDnnHandle, None, 4, pool.handle, dq.data_ptr(), None) == api.FDNN_E_ARG
    torch.cuda.synchronize()
    assert api.pool_launches() == before and (dq == -7.0).all()
    assert dnn.calculatePool(x[:0], pool).shape == (0, C)  # n == 0: nothing to do
    for p in (pool, narrow, wide):
        p.delete()
    ctx.delete()


def test_a_call_of_two_chunks_equals_two_calls(nets):
    dnn, _, dense = nets("mid")
    n = 20480 + 300
    for chained in (True, False):
        assert len(api.frame_chunks(n, chained)) >= 2
    x = F.synth_features(n, 432, seed=1600)
    co, C = PC.map_of("interleaved", dense.shape[1])
    pool = api.ClassPool(co, C)
    got = dnn.calculatePool(x, pool)
    cut = api.frame_chunks(n, True)[1][0]
    a, b = dnn.calculatePool(x[:cut], pool), dnn.calculatePool(x[cut:], pool)
    assert PC.same_bytes(got, np.concatenate([a, b]))
    rows = [0, 1, cut - 1, cut, n - 1]  # ... which are the pool of the dense rows
    assert PC.same_bytes(got[rows], api.pool_ref(dnn.calculate(x[rows]), co, C))
    pool.delete()


def test_a_device_call_of_two_chunks_equals_two_calls(nets):
    import torch

    dnn, _, dense = nets("tiny")
    n = 20480 + 1
    for chained in (True, False):
        assert len(api.frame_chunks(n, chained)) == 2
    cut = api.frame_chunks(n, True)[1][0]
    co, C = PC.map_of("quarter_out", dense.shape[1])
    pool = api.ClassPool(co, C)
    x = F.synth_features(n, 432, seed=1601)
    dx = torch.from_numpy(x).cuda()
    dq = torch.full((n * C + 4,), -7.0, dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    dnn.calculate_pool_device(dx.data_ptr(), n, pool, dq.data_ptr(), st.cuda_stream)
    st.synchronize()
    assert (dq[n * C:] == -7.0).all()
    want = np.concatenate([dnn.calculatePool(x[:cut], pool), dnn.calculatePool(x[cut:], pool)])
    assert PC.same_bytes(dq[:n * C].cpu().numpy().reshape(n, C), want)
    pool.delete()


def test_a_hidden_only_stream_push(nets):
    dnn, _, dense0 = nets("mid")
    co, C = PC.map_of("interleaved", dense0.shape[1])
    pool = api.ClassPool(co, C)
    dnn.setSplice(*KALDI)
    try:
        raw = (np.random.default_rng(88).standard_normal((90, 39)) * 3).astype(np.float32)
        dense = dnn.calculateRaw(raw)
        st = dnn.newStream(64)
        got, done = [], 0
        for i in (0, 64):
            ctx = st.pushHidden(raw[i:i + 64], end=i + 64 >= len(raw))
            rows = ctx.inputVectorCount
            got.append((ctx.calculateOutputPool(pool), done, rows))
            done += rows
        st.close()
        assert done == len(raw)
        for res, first, rows in got:
            assert rows > 0 and PC.same_bytes(res, api.pool_ref(dense[first:first + rows], co, C))
    finally:
        dnn.setSplice([], 0)
        pool.delete()


@pytest.mark.parametrize("net", ["tiny", "mid", "full"])
def test_against_the_oracle_on_every_row(nets, fixtures, net):
    """|q_c - sum| <= L_c 2e-6 + d_c u / (1 - d_c u) (sum + L_c 2e-6): the project's absolute bar per probability plus the
    derived bound of the additions; with every node mapped the class sums add up to the row's float64 total within the same
    terms."""
    dnn, x, _ = nets(net)
    orc = Oracle(LC.model_path(net, fixtures))
    p = orc.output_mt(orc.hidden_acts_mt(x)).astype(np.float64)
    assert np.isfinite(p).all()
    n, O = p.shape
    for mk in ("interleaved", "blocks", "sizes", "one"):
        co, C = PC.map_of(mk, O)
        pool = api.ClassPool(co, C)
        q = dnn.calculatePool(x, pool).astype(np.float64)
        pool.delete()
        total_bound = np.zeros(n)
        worst = 0.0
        for c, m in enumerate(PC.members(co, C)):
            exact = p[:, m].sum(1)
            bound = PC.oracle_bound(m.size, exact, LC.TIGHT)
            err = np.abs(q[:, c] - exact)
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if m.size else 0.0)
            assert (err <= bound).all(), (net, mk, c, m.size, float(err.max()), float(bound.min()))
            total_bound += bound
        print(f"{net} {mk}: largest |q - oracle sum| / bound = {worst:.3f}")
        if (co >= 0).all():
            assert (np.abs(q.sum(1) - p.sum(1)) <= total_bound).all(), (net, mk)
