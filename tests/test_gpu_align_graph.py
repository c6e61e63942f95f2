"""Alignment graphs through the model (fdnn_calculate_align_graph and its raw-frame, context and device-result forms), on the
nets of tests/test_gpu_align.py: every entry point's path and total are the host restatement's (api.align_graph_ref, held to
numpy and to brute force by tests/test_align_graph_host.py) over the bytes that fdnn_calculate_lazy_sets returns for the
graphs' node sets (api.align_sets), turned into scores by api.loglik_entries_ref -- the lazy path is untouched, so the
composition is exact.  The transcripts are api.optional_silence_graph's."""
import numpy as np
import pytest

import align_cases as AC
import align_graph_cases as GC
import lazy_lists_cases as LC
import loglik_cases as LL
from fast_dnn_amd import api, convert, formats as F

pytestmark = pytest.mark.gpu
FAR = GC.FAR
silence_node, silence_graphs, composed, not_blind = GC.silence_node, GC.silence_graphs, GC.composed, GC.not_blind  # (shared with tests/test_gpu_signal_nets.py)
same, seg_rows_of = AC.same, AC.seg_rows_of
KALDI = (list(range(-5, 6)), 39)
NETS = {"tiny": (33, 1), "mid": (100, 3), "full": (64, 2)}  # net -> frames, segments
HANDLES = ((-20.0, api.LOGLIK_F32), (-20.0, api.LOGLIK_F16))
SIL = 0  # the silence node of the hand-written graphs (the transcripts from a net's rows take the rows' most frequent argmax)


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
    graphs = silence_graphs(dense, seg_rows, 31)
    packed = api.pack_graphs(graphs)
    lp = LL.priors(O)
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutput(x)
    st = torch.cuda.Stream()
    for handle in HANDLES:
        ll = api.Loglik(lp, *handle)
        want, pieces = composed(dnn, x, lp, handle, seg_rows, packed)
        assert np.isfinite(want[1]).all()
        not_blind(net, want, pieces, seg_rows, graphs)
        before = api.align_graph_launches(), api.align_launches()
        assert same(dnn.calculateAlignGraph(x, ll, seg_rows, packed), want), (net, handle)
        assert sum(api.align_graph_launches()) == sum(before[0]) + 1 and api.align_launches() == before[1]  # a counter of their own
        assert same(ctx.alignGraph(ll, seg_rows, packed), want), (net, handle)
        for mode in (1, 2):
            api.set_align_graph_kernel(mode)
            try:
                assert same(ctx.alignGraph(ll, seg_rows, packed), want), (net, handle, mode)
            finally:
                api.set_align_graph_kernel(0)
        d_path = torch.full((n + 8,), -7, dtype=torch.int32, device="cuda")
        d_total = torch.full((seg_rows.size - 1 + 8,), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.alignGraphDevice(ll, seg_rows, packed, d_path.data_ptr() + 16, d_total.data_ptr() + 16, st.cuda_stream)
        st.synchronize()
        p, t = d_path.cpu().numpy(), d_total.cpu().numpy()
        assert (p[:4] == -7).all() and (p[4 + n:] == -7).all() and (t[:4] == -7).all() and (t[-4:] == -7).all()
        assert same((p[4:4 + n], t[4:-4]), want)
        # the default start and final states, and a part of the context's rows
        plain = api.pack_graphs([dict(g, start_lp=None, final_lp=None) for g in graphs])
        assert plain["startLp"] is None and same(ctx.alignGraph(ll, seg_rows, plain), composed(dnn, x, lp, handle, seg_rows, plain)[0])
        if seg_rows.size > 2:
            a, b = int(seg_rows[1]), int(seg_rows[2])
            part = ctx.alignGraph(ll, seg_rows[1:3], api.pack_graphs(graphs[1:2]))
            assert np.array_equal(part[0], want[0][a:b]) and part[1].view(np.uint32)[0] == want[1].view(np.uint32)[1]
        # the chain as a graph through the model: fdnn_calculate_align's bytes
        sp = packed["statePtr"]
        sl, nl = AC.transitions(int(sp[-1]), 32)
        chains = api.pack_graphs([api.chain_graph(g["states"], sl[sp[s]:sp[s + 1]], nl[sp[s]:sp[s + 1]]) for s, g in enumerate(graphs)])
        assert same(dnn.calculateAlignGraph(x, ll, seg_rows, chains), dnn.calculateAlign(x, ll, seg_rows, sp, packed["states"], sl, nl))
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
        packed = api.pack_graphs(silence_graphs(dense, seg_rows, 42))
        ll = api.Loglik(LL.priors(dense.shape[1]), -20.0, api.LOGLIK_F16)
        got = dnn.calculateAlignGraphRaw(raw, ll, seg_rows, packed)
        assert np.isfinite(got[1]).all() and same(got, dnn.calculateAlignGraph(x, ll, seg_rows, packed))
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
    graphs = []
    for n_words in (8, 12, 6):
        words = [rng.integers(1, dense.shape[1], 4).tolist() for _ in range(n_words)]
        g = api.optional_silence_graph(words, SIL)
        g["arc_lp"] = np.log(rng.uniform(0.05, 0.95, g["arc_lp"].size)).astype(np.float32)
        graphs.append(g)
    packed = api.pack_graphs(graphs)
    lp = LL.priors(dense.shape[1])
    handle = (-20.0, api.LOGLIK_F16)
    ll = api.Loglik(lp, *handle)
    before = api.align_graph_launches()
    got = dnn.calculateAlignGraph(x, ll, seg_rows, packed)
    assert sum(api.align_graph_launches()) == sum(before) + 1  # the recursion runs ONCE, behind the last chunk
    assert np.isfinite(got[1]).all()
    a, b = int(seg_rows[1]), int(seg_rows[2])
    alone = dnn.calculateAlignGraph(x[a:b], ll, [0, b - a], api.pack_graphs(graphs[1:2]))  # one chunk
    assert np.array_equal(got[0][a:b], alone[0]) and got[1].view(np.uint32)[1] == alone[1].view(np.uint32)[0]
    assert same(got, composed(dnn, x, lp, handle, seg_rows, packed)[0])
    ll.delete()


def test_state_and_argument_errors(nets):
    dnn, x, dense = nets("tiny")
    n, O = dense.shape
    ll = api.Loglik(LL.priors(O), -20.0, api.LOGLIK_F16)
    narrow = api.Loglik(np.zeros(O - 1, np.float32))
    seg_rows = np.array([0, 20, n], np.int32)
    ga, gb = api.optional_silence_graph([[1, 2]], SIL), api.optional_silence_graph([[3], [4, 5]], SIL)  # 4 and 6 states, 7 and 12 arcs
    good = api.pack_graphs([ga, gb])
    assert good["statePtr"].tolist() == [0, 4, 10] and good["arcPtr"][-1] == 19
    ctx = dnn.getNewLazyContext(n)
    with pytest.raises(api.FdnnError) as e:
        ctx.alignGraph(ll, seg_rows, good)  # before the hidden layers
    assert e.value.code == api.FDNN_E_STATE
    ctx.calculateUntilOutput(x)
    assert np.isfinite(ctx.alignGraph(ll, seg_rows, good)[1]).all()
    before = api.align_graph_launches(), api.sets_launches()

    def refused(text, ll_=ll, rows=seg_rows, **change):
        g = dict(good)
        for key, (at, value) in change.items():
            g[key] = np.array(g[key])
            g[key][at] = value
        for call in (lambda: dnn.calculateAlignGraph(x, ll_, rows, g), lambda: ctx.alignGraph(ll_, rows, g)):
            with pytest.raises(api.FdnnError) as e:
                call()
            assert e.value.code == api.FDNN_E_ARG and text in str(e.value), (text, str(e.value))

    refused("width", ll_=narrow)
    refused("segment 1", rows=np.array([0, 20, 20], np.int32))     # a segment without rows
    refused("segment 1", rows=np.array([0, 20, n + 1], np.int32))  # past the context
    refused("segment 1", states=(6, O))                            # a node outside the layer
    refused("segment 0", states=(1, -1))
    refused("segment 0", statePtr=(1, 0))                          # a graph without states
    refused("segment 0", arcPtr=(0, 1))                            # arc_ptr does not begin at 0
    refused("segment 1", arcPtr=(6, 2))                            # ... decreases
    refused("segment 0", arcSrc=(2, 4))                            # a source outside [0, S): S = 4
    refused("segment 1", arcSrc=(9, -1))
    refused("segment 1", arcLp=(12, np.inf))
    refused("segment 0", arcLp=(0, np.nan))
    refused("segment 1", startLp=(5, np.nan))
    refused("segment 0", finalLp=(0, np.inf))
    refused("no state has a finite start", startLp=(slice(0, 4), -np.inf))
    refused("no state has a finite final", finalLp=(slice(4, 10), -np.inf))
    with pytest.raises(api.FdnnError) as e:
        dnn.calculateAlignGraph(x, ll, np.array([0, 20, n - 1], np.int32), good)  # seg_rows must cover [0, n)
    assert e.value.code == api.FDNN_E_ARG
    with pytest.raises(api.FdnnError) as e:
        dnn.calculateAlignGraphRaw(np.zeros((n, 39), np.float32), ll, seg_rows, good)  # no splice spec
    assert e.value.code == api.FDNN_E_STATE
    L = api.lib()
    i32, f32 = api.C.POINTER(api.C.c_int), api.C.POINTER(api.C.c_float)
    path, total = np.empty(n, np.int32), np.empty(2, np.float32)
    ip, fp = (lambda a: a.ctypes.data_as(i32)), (lambda a: a.ctypes.data_as(f32))
    args = (ip(seg_rows), ip(good["statePtr"]), 2, ip(good["states"]), ip(good["arcPtr"]), ip(good["arcSrc"]), fp(good["arcLp"]), fp(good["startLp"]),
            fp(good["finalLp"]))
    assert L.fdnn_ctx_align_graph(ctx.handle, None, *args, ip(path), fp(total)) == api.FDNN_E_ARG
    assert L.fdnn_ctx_align_graph(None, ll.handle, *args, ip(path), fp(total)) == api.FDNN_E_ARG
    assert L.fdnn_ctx_align_graph(ctx.handle, ll.handle, *args, None, fp(total)) == api.FDNN_E_ARG
    no_arcs = args[:4] + (None,) + args[5:]
    assert L.fdnn_ctx_align_graph(ctx.handle, ll.handle, *no_arcs, ip(path), fp(total)) == api.FDNN_E_ARG
    assert L.fdnn_calculate_align_graph(dnn.nativeDnnHandle, None, n, 432, ll.handle, *args, ip(path), fp(total)) == api.FDNN_E_ARG
    assert L.fdnn_calculate_align_graph(dnn.nativeDnnHandle, fp(x), n, 431, ll.handle, *args, ip(path), fp(total)) == api.FDNN_E_ARG
    assert (api.align_graph_launches(), api.sets_launches()) == before  # refused before anything was launched
    # T < S is no error for a graph: the four-state graph over two rows skips its silences
    assert np.isfinite(ctx.alignGraph(ll, np.array([0, 2, n], np.int32), good)[1]).all()
    p0, t0 = dnn.calculateAlignGraph(x[:0], ll, [0], api.pack_graphs([]))  # nothing to do
    assert p0.size == 0 and t0.size == 0
    for h in (ll, narrow):
        h.delete()
    ctx.delete()


def test_a_model_that_leads_a_device_group_is_refused(tiny_model_path):
    """FDNN_E_ARG before any launch: an align-graph call does not run on a model that leads a device group."""
    grp = api.DeviceGroup(tiny_model_path, [0, 0])
    lead = grp.model(0)
    api._check(api.lib().fdnn_group_attach(grp.handle))
    O = lead.outputDimension()
    ll = api.Loglik(LL.priors(O), -20.0, api.LOGLIK_F32)
    x = F.synth_features(20, 432, seed=2700)
    packed = api.pack_graphs([api.chain_graph([0, 1, 2, 3])])
    before = api.align_graph_launches(), api.sets_launches()
    ctx = lead.getNewLazyContext(20)
    ctx.calculateUntilOutput(x)
    for call in (lambda: lead.calculateAlignGraph(x, ll, [0, 20], packed), lambda: ctx.alignGraph(ll, [0, 20], packed)):
        with pytest.raises(api.FdnnError) as e:
            call()
        assert e.value.code == api.FDNN_E_ARG and "device group" in str(e.value), str(e.value)
    assert (api.align_graph_launches(), api.sets_launches()) == before
    ctx.delete()
    ll.delete()
    grp.delete()


def test_scratch_over_the_cap_is_refused_by_the_host_plan():
    """One segment of 2^19 + 1 frames and 1024 states needs more than 2^30 bytes of back-pointers (2 bytes a frame and state):
    FDNN_E_ARG from the plan, before any launch, nothing allocated; 2^19 frames pass the cap."""
    import torch

    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    L, i32, i64 = api.lib(), api.C.POINTER(api.C.c_int), api.C.POINTER(api.C.c_longlong)
    cap_words = api.align_graph_limits()["scratch_cap_mib"] * (1 << 20) // 4
    assert api.align_graph_scratch_words([1 << 19], [0, 1024]) == cap_words and api.align_graph_scratch_words([(1 << 19) + 1], [0, 1024]) == cap_words + 512
    before = api.align_graph_launches()
    ap = np.zeros(1025, np.int32)

    def call(T, scratch=0, words=0):
        a = [np.array(v, t) for v, t in (([T], np.int32), ([0], np.int64), ([8], np.int32), ([0, 1024], np.int32))]
        rc = L.fdnn_align_graph_rows_device(None, p, a[0].ctypes.data_as(i32), a[1].ctypes.data_as(i64), a[2].ctypes.data_as(i32), a[3].ctypes.data_as(i32),
                                            ap.ctypes.data_as(i32), 1, p, None, p, None, None, None, None, scratch, words, p, p, None)
        return rc, L.fdnn_last_error().decode(errors="replace")

    rc, msg = call((1 << 19) + 1, p, 1 << 40)  # (however much scratch the caller claims to bring)
    assert rc == api.FDNN_E_ARG and "above" in msg and str(1 << 30) in msg, msg
    rc, msg = call(1 << 19)  # passes the cap: the refusal is the missing scratch
    assert rc == api.FDNN_E_ARG and "fdnn_align_graph_scratch_words" in msg and str(cap_words) in msg, msg
    torch.cuda.synchronize()
    assert api.align_graph_launches() == before
