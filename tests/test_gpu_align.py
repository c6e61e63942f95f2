"""Forced alignment through the model (fdnn_calculate_align and its raw-frame, context and device-result forms), on nets of
tests/test_gpu_loglik.py: every entry point's path and total are the host restatement's (api.align_ref, held to numpy and to
brute force by tests/test_align_host.py) over the bytes that fdnn_calculate_lazy_sets returns for the transcripts' node sets
(api.align_sets), turned into scores by api.loglik_entries_ref -- the lazy path is untouched, so the composition is exact."""
import numpy as np
import pytest

import align_cases as AC
import lazy_lists_cases as LC
import loglik_cases as LL
from fast_dnn_amd import api, convert, formats as F

pytestmark = pytest.mark.gpu
transcripts, composed, same, seg_rows_of = AC.transcripts, AC.composed, AC.same, AC.seg_rows_of  # (shared with tests/test_gpu_signal_nets.py)
KALDI = (list(range(-5, 6)), 39)
NETS = {"tiny": (33, 1), "mid": (100, 3), "full": (64, 2)}  # net -> frames, segments
HANDLES = ((-20.0, api.LOGLIK_F32), (-20.0, api.LOGLIK_F16))


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
            x = F.synth_features(NETS[net][0], LC.in_dim(net), seed=2500 + len(net))
            cache[net] = (dnn, x, dnn.calculate(x))
        return cache[net]

    yield get
    for dnn, _, _ in cache.values():
        dnn.delete()


@pytest.mark.parametrize("net", list(NETS))
def test_every_entry_point_returns_the_restatements_path(nets, net):
    import torch

    dnn, x, dense = nets(net)
    n, O = dense.shape
    seg_rows = seg_rows_of(n, NETS[net][1])
    ptr, states = transcripts(dense, seg_rows, 31)
    assert (np.diff(ptr) < np.diff(seg_rows)).all() and np.unique(states).size < states.size
    sl, nl = AC.transitions(states.size, 32)
    lp = LL.priors(O)
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutput(x)
    st = torch.cuda.Stream()
    for handle in HANDLES:
        ll = api.Loglik(lp, *handle)
        want = composed(dnn, x, lp, handle, seg_rows, ptr, states, sl, nl)
        assert np.isfinite(want[1]).all()
        for s in range(seg_rows.size - 1):  # the comparison is not blind: the path is far from the uniform segmentation
            p = want[0][seg_rows[s]:seg_rows[s + 1]]
            frac = AC.differ(p, AC.uniform_path(p.size, int(ptr[s + 1] - ptr[s])))
            print(f"{net} segment {s}: T {p.size} S {ptr[s + 1] - ptr[s]}, {frac:.0%} of the frames off the uniform segmentation")
            assert frac >= 0.25
        before = api.align_launches()
        assert same(dnn.calculateAlign(x, ll, seg_rows, ptr, states, sl, nl), want), (net, handle)
        assert sum(api.align_launches()) == sum(before) + 1
        assert same(ctx.align(ll, seg_rows, ptr, states, sl, nl), want), (net, handle)
        for mode in (1, 2):
            api.set_align_kernel(mode)
            try:
                assert same(ctx.align(ll, seg_rows, ptr, states, sl, nl), want), (net, handle, mode)
            finally:
                api.set_align_kernel(0)
        d_path = torch.full((n + 8,), -7, dtype=torch.int32, device="cuda")
        d_total = torch.full((seg_rows.size - 1 + 8,), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.alignDevice(ll, seg_rows, ptr, states, d_path.data_ptr() + 16, d_total.data_ptr() + 16, sl, nl, st.cuda_stream)
        st.synchronize()
        p, t = d_path.cpu().numpy(), d_total.cpu().numpy()
        assert (p[:4] == -7).all() and (p[4 + n:] == -7).all() and (t[:4] == -7).all() and (t[-4:] == -7).all()
        assert same((p[4:4 + n], t[4:-4]), want)
        # without transitions, and a part of the context's rows
        assert same(ctx.align(ll, seg_rows, ptr, states), composed(dnn, x, lp, handle, seg_rows, ptr, states, None, None))
        if seg_rows.size > 2:
            a, b = int(seg_rows[1]), int(seg_rows[2])
            part = ctx.align(ll, seg_rows[1:3], ptr[1:3] - ptr[1], states[ptr[1]:ptr[2]], sl[ptr[1]:ptr[2]], nl[ptr[1]:ptr[2]])
            assert np.array_equal(part[0], want[0][a:b]) and part[1].view(np.uint32)[0] == want[1].view(np.uint32)[1]
        ll.delete()
    ctx.delete()
    assert np.array_equal(dnn.calculate(x).view(np.uint32), dense.view(np.uint32))  # the dense entry point keeps its bytes


def test_raw_frames_equal_spliced_rows(nets):
    dnn, _, _ = nets("mid")
    dnn.setSplice(*KALDI)
    try:
        raw = (np.random.default_rng(41).standard_normal((90, 39)) * 3).astype(np.float32)
        seg_rows = np.array([0, 50, 90], np.int32)
        x = np.concatenate([convert.splice_frames(raw[a:b], KALDI[0], 432) for a, b in zip(seg_rows[:-1], seg_rows[1:])])  # every segment an utterance of its own
        dense = dnn.calculate(x)
        ptr, states = transcripts(dense, seg_rows, 42)
        sl, nl = AC.transitions(states.size, 43)
        ll = api.Loglik(LL.priors(dense.shape[1]), -20.0, api.LOGLIK_F16)
        got = dnn.calculateAlignRaw(raw, ll, seg_rows, ptr, states, sl, nl)
        assert np.isfinite(got[1]).all() and same(got, dnn.calculateAlign(x, ll, seg_rows, ptr, states, sl, nl))
        ll.delete()
    finally:
        dnn.setSplice([], 0)


def test_two_chunks_that_cut_a_segment_give_the_uncut_path(nets):
    dnn, _, dense = nets("mid")
    n = 20480 + 300
    for chained in (True, False):
        assert len(api.frame_chunks(n, chained)) == 2
    cut = api.frame_chunks(n, True)[1][0]
    seg_rows = np.array([0, cut - 80, cut + 120, n], np.int32)  # the middle segment is cut by the chunk
    x = F.synth_features(n, 432, seed=2600)
    rng = np.random.default_rng(44)
    ptr = np.array([0, 30, 80, 100], np.int32)
    states = rng.integers(0, dense.shape[1], 100).astype(np.int32)
    sl, nl = AC.transitions(100, 45)
    lp = LL.priors(dense.shape[1])
    handle = (-20.0, api.LOGLIK_F16)
    ll = api.Loglik(lp, *handle)
    before = api.align_launches()
    got = dnn.calculateAlign(x, ll, seg_rows, ptr, states, sl, nl)
    assert sum(api.align_launches()) == sum(before) + 1  # the recursion runs ONCE, behind the last chunk
    assert np.isfinite(got[1]).all()
    a, b = int(seg_rows[1]), int(seg_rows[2])
    alone = dnn.calculateAlign(x[a:b], ll, [0, b - a], [0, 50], states[30:80], sl[30:80], nl[30:80])  # one chunk
    assert np.array_equal(got[0][a:b], alone[0]) and got[1].view(np.uint32)[1] == alone[1].view(np.uint32)[0]
    assert same(got, composed(dnn, x, lp, handle, seg_rows, ptr, states, sl, nl))
    ll.delete()


def test_the_ctx_form_after_a_hidden_only_stream_push(nets):
    dnn, _, dense0 = nets("mid")
    lp = LL.priors(dense0.shape[1])
    handle = (-20.0, api.LOGLIK_F32)
    ll = api.Loglik(lp, *handle)
    dnn.setSplice(*KALDI)
    try:
        raw = (np.random.default_rng(46).standard_normal((60, 39)) * 3).astype(np.float32)
        st = dnn.newStream(64)
        ctx = st.pushHidden(raw, end=True)
        n = ctx.inputVectorCount
        assert n == 60
        dense = dnn.calculateRaw(raw)
        seg_rows = np.array([0, n], np.int32)
        ptr, states = transcripts(dense, seg_rows, 47)
        sl, nl = AC.transitions(states.size, 48)
        got = ctx.align(ll, seg_rows, ptr, states, sl, nl)
        st.close()
        want = dnn.calculateAlignRaw(raw, ll, seg_rows, ptr, states, sl, nl)  # the same rows, spliced by the one-call form
        assert np.isfinite(want[1]).all() and same(got, want)
    finally:
        dnn.setSplice([], 0)
        ll.delete()


def test_state_and_argument_errors(nets):
    dnn, x, dense = nets("tiny")
    n, O = dense.shape
    ll = api.Loglik(LL.priors(O), -20.0, api.LOGLIK_F16)
    narrow = api.Loglik(np.zeros(O - 1, np.float32))
    seg_rows, ptr, states = np.array([0, 20, n], np.int32), np.array([0, 4, 9], np.int32), np.arange(9, dtype=np.int32)
    zeros = np.zeros(9, np.float32)
    ctx = dnn.getNewLazyContext(n)
    with pytest.raises(api.FdnnError) as e:
        ctx.align(ll, seg_rows, ptr, states)  # before the hidden layers
    assert e.value.code == api.FDNN_E_STATE
    ctx.calculateUntilOutput(x)
    last = zeros.copy()
    last[[3, 8]] = np.nan  # next_lp of a last state is never read
    assert np.isfinite(ctx.align(ll, seg_rows, ptr, states, zeros, last)[1]).all()
    before = api.align_launches(), api.sets_launches()

    def refused(text, ll_=ll, rows=seg_rows, p=ptr, st=states, sl=None, nl=None):
        for call in (lambda: dnn.calculateAlign(x, ll_, rows, p, st, sl, nl), lambda: ctx.align(ll_, rows, p, st, sl, nl)):
            with pytest.raises(api.FdnnError) as e:
                call()
            assert e.value.code == api.FDNN_E_ARG and text in str(e.value), (text, str(e.value))

    refused("width", ll_=narrow)
    refused("segment 1", rows=np.array([0, 20, 20], np.int32))              # a segment without rows
    refused("segment 1", rows=np.array([0, 20, n + 1], np.int32))           # past the context
    refused("segment 1", st=np.array([0, 1, 2, 3, 4, 5, O, 7, 8], np.int32))  # a node outside the layer
    refused("segment 0", st=np.array([0, -1, 2, 3, 4, 5, 6, 7, 8], np.int32))
    refused("segment 0", p=np.array([0, 0, 9], np.int32))                   # a transcript without states
    refused("segment 1", rows=np.array([0, n - 3, n], np.int32))            # T < S
    bad = zeros.copy()
    bad[5] = np.inf
    refused("segment 1", sl=bad)
    bad = zeros.copy()
    bad[2] = np.nan
    refused("segment 0", nl=bad)
    with pytest.raises(api.FdnnError) as e:
        dnn.calculateAlign(x, ll, np.array([0, 20, n - 1], np.int32), ptr, states)  # seg_rows must cover [0, n)
    assert e.value.code == api.FDNN_E_ARG
    with pytest.raises(api.FdnnError) as e:
        dnn.calculateAlignRaw(np.zeros((n, 39), np.float32), ll, seg_rows, ptr, states)  # no splice spec
    assert e.value.code == api.FDNN_E_STATE
    L = api.lib()
    i32, f32 = api.C.POINTER(api.C.c_int), api.C.POINTER(api.C.c_float)
    path, total = np.empty(n, np.int32), np.empty(2, np.float32)
    args = (seg_rows.ctypes.data_as(i32), ptr.ctypes.data_as(i32), 2, states.ctypes.data_as(i32), None, None)
    assert L.fdnn_ctx_align(ctx.handle, None, *args, path.ctypes.data_as(i32), total.ctypes.data_as(f32)) == api.FDNN_E_ARG
    assert L.fdnn_ctx_align(None, ll.handle, *args, path.ctypes.data_as(i32), total.ctypes.data_as(f32)) == api.FDNN_E_ARG
    assert L.fdnn_ctx_align(ctx.handle, ll.handle, *args, None, total.ctypes.data_as(f32)) == api.FDNN_E_ARG
    assert L.fdnn_calculate_align(dnn.nativeDnnHandle, None, n, 432, ll.handle, *args, path.ctypes.data_as(i32), total.ctypes.data_as(f32)) == api.FDNN_E_ARG
    assert L.fdnn_calculate_align(dnn.nativeDnnHandle, x.ctypes.data_as(f32), n, 431, ll.handle, *args, path.ctypes.data_as(i32),
                                  total.ctypes.data_as(f32)) == api.FDNN_E_ARG
    assert (api.align_launches(), api.sets_launches()) == before  # refused before anything was launched
    p0, t0 = dnn.calculateAlign(x[:0], ll, [0], [0], [])  # nothing to do
    assert p0.size == 0 and t0.size == 0
    for h in (ll, narrow):
        h.delete()
    ctx.delete()


def test_a_model_that_leads_a_device_group_is_refused(tiny_model_path):
    """FDNN_E_ARG before any launch: an align call does not run on a model that leads a device group (two replicas on one card)."""
    grp = api.DeviceGroup(tiny_model_path, [0, 0])
    lead = grp.model(0)
    api._check(api.lib().fdnn_group_attach(grp.handle))
    O = lead.outputDimension()
    ll = api.Loglik(LL.priors(O), -20.0, api.LOGLIK_F32)
    x = F.synth_features(20, 432, seed=2700)
    seg_rows, ptr, states = [0, 20], [0, 4], [0, 1, 2, 3]
    before = api.align_launches(), api.sets_launches()
    ctx = lead.getNewLazyContext(20)
    ctx.calculateUntilOutput(x)
    for call in (lambda: lead.calculateAlign(x, ll, seg_rows, ptr, states), lambda: ctx.align(ll, seg_rows, ptr, states)):
        with pytest.raises(api.FdnnError) as e:
            call()
        assert e.value.code == api.FDNN_E_ARG and "device group" in str(e.value), str(e.value)
    assert (api.align_launches(), api.sets_launches()) == before
    ctx.delete()
    ll.delete()
    grp.delete()


def test_scratch_over_the_cap_is_refused_by_the_host_plan():
    """One segment of 2^23 + 1 frames and 1024 states (sixteen states a lane, 32 take words a frame) needs more than 2^30 bytes
    of back-pointer words: FDNN_E_ARG from the plan, before any launch, nothing allocated; 2^23 frames pass the cap."""
    import torch

    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    L, i32, i64 = api.lib(), api.C.POINTER(api.C.c_int), api.C.POINTER(api.C.c_longlong)
    cap_words = api.align_limits()["scratch_cap_mib"] * (1 << 20) // 4
    assert api.align_scratch_words([1 << 23], [0, 1024]) == cap_words and api.align_scratch_words([(1 << 23) + 1], [0, 1024]) == cap_words + 32
    before = api.align_launches()

    def call(T, scratch=0, words=0):
        a = [np.array(v, t) for v, t in (([T], np.int32), ([0], np.int64), ([8], np.int32), ([0, 1024], np.int32))]
        rc = L.fdnn_align_rows_device(None, p, a[0].ctypes.data_as(i32), a[1].ctypes.data_as(i64), a[2].ctypes.data_as(i32), a[3].ctypes.data_as(i32), 1,
                                      p, None, None, None, scratch, words, p, p, None)
        return rc, L.fdnn_last_error().decode(errors="replace")

    rc, msg = call((1 << 23) + 1, p, 1 << 40)  # (however much scratch the caller claims to bring)
    assert rc == api.FDNN_E_ARG and "above" in msg and str(1 << 30) in msg, msg
    rc, msg = call(1 << 23)  # passes the cap: the refusal is the missing scratch
    assert rc == api.FDNN_E_ARG and "fdnn_align_scratch_words" in msg and str(cap_words) in msg, msg
    torch.cuda.synchronize()
    assert api.align_launches() == before
