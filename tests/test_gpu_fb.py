"""Forward-backward over alignment graphs through the model (fdnn_calculate_fb and its raw-frame, context and device-result
forms), on the nets of tests/test_gpu_align_graph.py: every entry point's total and gamma are the host restatement's
(api.fb_ref, held to float64 and to brute force by tests/test_fb_host.py) over the bytes that fdnn_calculate_lazy_sets returns
for the graphs' node sets (api.align_sets), turned into scores by api.loglik_entries_ref -- the lazy path is untouched, so the
composition is exact.  The transcripts are api.optional_silence_graph's."""
import numpy as np
import pytest

import align_cases as AC
import align_graph_cases as GC
import lazy_lists_cases as LC
import loglik_cases as LL
from fast_dnn_amd import api, convert, formats as F

pytestmark = pytest.mark.gpu
seg_rows_of = AC.seg_rows_of
KALDI = (list(range(-5, 6)), 39)
NETS = {"tiny": (33, 1), "mid": (100, 3)}  # net -> frames, segments
HANDLES = ((-20.0, api.LOGLIK_F32), (-20.0, api.LOGLIK_F16))
SIL = 0


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


def same(got, want):
    ok = np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    if want[1] is None:
        return ok and got[1] is None
    return ok and got[1] is not None and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def composed(dnn, x, lp, handle, seg_rows, packed, want_gamma=True):
    """The restatement over the lazy sets call's bytes -> (total, gamma)."""
    _, (e, T, off, ln, col) = GC.composed(dnn, x, lp, handle, seg_rows, packed)
    return api.fb_ref(e, T, off, ln, packed, col, want_gamma=want_gamma)


@pytest.mark.parametrize("net", list(NETS))
def test_every_entry_point_returns_the_restatements_bytes(nets, net):
    import torch

    dnn, x, dense = nets(net)
    n, O = dense.shape
    seg_rows = seg_rows_of(n, NETS[net][1])
    graphs = GC.silence_graphs(dense, seg_rows, 31)
    packed = api.pack_graphs(graphs)
    cells = int((np.diff(seg_rows).astype(np.int64) * np.diff(packed["statePtr"])).sum())
    lp = LL.priors(O)
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutput(x)
    st = torch.cuda.Stream()
    for handle in HANDLES:
        ll = api.Loglik(lp, *handle)
        want = composed(dnn, x, lp, handle, seg_rows, packed)
        fwd = composed(dnn, x, lp, handle, seg_rows, packed, want_gamma=False)
        best = GC.composed(dnn, x, lp, handle, seg_rows, packed)[0][1]
        assert np.isfinite(want[0]).all() and (want[0] >= best).all() and want[1].size == cells
        blocks = api.fb_gamma_blocks(want[1], np.diff(seg_rows), packed["statePtr"])
        soft = np.mean([(b.max(axis=1) < 0.9).mean() for b in blocks])
        print(f"{net} {handle}: total - best path {np.round(want[0] - best, 3).tolist()}, {soft:.0%} of the frames have max gamma < 0.9")
        assert all((np.abs(b.sum(axis=1, dtype=np.float64) - 1) < 1e-3).all() for b in blocks) and (want[0] > best).any() and soft > 0
        before = api.fb_launches(), api.align_graph_launches()
        assert same(dnn.calculateForwardBackward(x, ll, seg_rows, packed), want), (net, handle)
        assert sum(api.fb_launches()) == sum(before[0]) + 2 and api.align_graph_launches() == before[1]  # a counter of their own
        mid = api.fb_launches()
        assert same(dnn.calculateForwardBackward(x, ll, seg_rows, packed, want_gamma=False), fwd)
        after = api.fb_launches()
        assert sum(after[:2]) == sum(mid[:2]) + 1 and after[2:] == mid[2:]  # forward only: no backward launch
        assert same(ctx.forwardBackward(ll, seg_rows, packed), want), (net, handle)
        assert same(ctx.forwardBackward(ll, seg_rows, packed, want_gamma=False), fwd)
        for mode in (1, 2):
            api.set_fb_kernel(mode)
            try:
                assert same(ctx.forwardBackward(ll, seg_rows, packed), want), (net, handle, mode)
            finally:
                api.set_fb_kernel(0)
        n_segs = seg_rows.size - 1
        d_gamma = torch.full((cells + 8,), -7.0, dtype=torch.float32, device="cuda")
        d_total = torch.full((n_segs + 8,), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.forwardBackwardDevice(ll, seg_rows, packed, d_total.data_ptr() + 16, d_gamma.data_ptr() + 16, st.cuda_stream)
        st.synchronize()
        gm, t = d_gamma.cpu().numpy(), d_total.cpu().numpy()
        assert (gm[:4] == -7).all() and (gm[4 + cells:] == -7).all() and (t[:4] == -7).all() and (t[-4:] == -7).all()
        assert same((t[4:-4], gm[4:4 + cells]), want)
        d_total.fill_(-7.0)
        ctx.forwardBackwardDevice(ll, seg_rows, packed, d_total.data_ptr() + 16, 0, st.cuda_stream)
        st.synchronize()
        assert same((d_total.cpu().numpy()[4:-4], None), fwd)
        # the default start and final states, and a part of the context's rows
        plain = api.pack_graphs([dict(g, start_lp=None, final_lp=None) for g in graphs])
        assert plain["startLp"] is None and same(ctx.forwardBackward(ll, seg_rows, plain), composed(dnn, x, lp, handle, seg_rows, plain))
        if seg_rows.size > 2:
            part = ctx.forwardBackward(ll, seg_rows[1:3], api.pack_graphs(graphs[1:2]))
            assert part[0].view(np.uint32)[0] == want[0].view(np.uint32)[1] and np.array_equal(part[1].view(np.uint32), blocks[1].ravel().view(np.uint32))
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
        packed = api.pack_graphs(GC.silence_graphs(dense, seg_rows, 42))
        ll = api.Loglik(LL.priors(dense.shape[1]), -20.0, api.LOGLIK_F16)
        got = dnn.calculateForwardBackwardRaw(raw, ll, seg_rows, packed)
        assert np.isfinite(got[0]).all() and same(got, dnn.calculateForwardBackward(x, ll, seg_rows, packed))
        fwd = dnn.calculateForwardBackwardRaw(raw, ll, seg_rows, packed, want_gamma=False)
        assert fwd[1] is None and np.array_equal(fwd[0].view(np.uint32), got[0].view(np.uint32))
        ll.delete()
    finally:
        dnn.setSplice([], 0)


def test_two_chunks_that_cut_a_segment_give_the_uncut_bytes(nets):
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
    before = api.fb_launches()
    got = dnn.calculateForwardBackward(x, ll, seg_rows, packed)
    delta = tuple(b - a for a, b in zip(before, api.fb_launches()))
    assert sum(delta[:2]) == 1 and sum(delta[2:]) == 1  # the sweeps run ONCE, behind the last chunk: one forward and one backward launch
    assert np.isfinite(got[0]).all()
    a, b = int(seg_rows[1]), int(seg_rows[2])
    alone = dnn.calculateForwardBackward(x[a:b], ll, [0, b - a], api.pack_graphs(graphs[1:2]))  # one chunk
    blocks = api.fb_gamma_blocks(got[1], np.diff(seg_rows), packed["statePtr"])
    assert got[0].view(np.uint32)[1] == alone[0].view(np.uint32)[0] and np.array_equal(blocks[1].ravel().view(np.uint32), alone[1].view(np.uint32))
    assert same(got, composed(dnn, x, lp, handle, seg_rows, packed))
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
        ctx.forwardBackward(ll, seg_rows, good)  # before the hidden layers
    assert e.value.code == api.FDNN_E_STATE
    ctx.calculateUntilOutput(x)
    assert np.isfinite(ctx.forwardBackward(ll, seg_rows, good)[0]).all()
    before = api.fb_launches(), api.sets_launches()

    def refused(text, ll_=ll, rows=seg_rows, **change):
        g = dict(good)
        for key, (at, value) in change.items():
            g[key] = np.array(g[key])
            g[key][at] = value
        for call in (lambda: dnn.calculateForwardBackward(x, ll_, rows, g), lambda: ctx.forwardBackward(ll_, rows, g),
                     lambda: ctx.forwardBackward(ll_, rows, g, want_gamma=False)):
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
        dnn.calculateForwardBackward(x, ll, np.array([0, 20, n - 1], np.int32), good)  # seg_rows must cover [0, n)
    assert e.value.code == api.FDNN_E_ARG
    with pytest.raises(api.FdnnError) as e:
        dnn.calculateForwardBackwardRaw(np.zeros((n, 39), np.float32), ll, seg_rows, good)  # no splice spec
    assert e.value.code == api.FDNN_E_STATE
    L = api.lib()
    i32, f32 = api.C.POINTER(api.C.c_int), api.C.POINTER(api.C.c_float)
    gamma, total = np.empty(20 * 4 + (n - 20) * 6, np.float32), np.empty(2, np.float32)
    ip, fp = (lambda a: a.ctypes.data_as(i32)), (lambda a: a.ctypes.data_as(f32))
    args = (ip(seg_rows), ip(good["statePtr"]), 2, ip(good["states"]), ip(good["arcPtr"]), ip(good["arcSrc"]), fp(good["arcLp"]), fp(good["startLp"]),
            fp(good["finalLp"]))
    assert L.fdnn_ctx_fb(ctx.handle, None, *args, fp(total), fp(gamma)) == api.FDNN_E_ARG
    assert L.fdnn_ctx_fb(None, ll.handle, *args, fp(total), fp(gamma)) == api.FDNN_E_ARG
    assert L.fdnn_ctx_fb(ctx.handle, ll.handle, *args, None, fp(gamma)) == api.FDNN_E_ARG
    no_arcs = args[:4] + (None,) + args[5:]
    assert L.fdnn_ctx_fb(ctx.handle, ll.handle, *no_arcs, fp(total), fp(gamma)) == api.FDNN_E_ARG
    assert L.fdnn_calculate_fb(dnn.nativeDnnHandle, None, n, 432, ll.handle, *args, fp(total), fp(gamma)) == api.FDNN_E_ARG
    assert L.fdnn_calculate_fb(dnn.nativeDnnHandle, fp(x), n, 431, ll.handle, *args, fp(total), fp(gamma)) == api.FDNN_E_ARG
    assert (api.fb_launches(), api.sets_launches()) == before  # refused before anything was launched
    # T < S is no error for a graph: the four-state graph over two rows skips its silences
    assert np.isfinite(ctx.forwardBackward(ll, np.array([0, 2, n], np.int32), good)[0]).all()
    t0, g0 = dnn.calculateForwardBackward(x[:0], ll, [0], api.pack_graphs([]))  # nothing to do
    assert t0.size == 0 and g0.size == 0
    for h in (ll, narrow):
        h.delete()
    ctx.delete()


def test_a_lattice_over_the_cap_is_refused_by_the_host_plan():
    """One segment of 2^18 + 1 frames and 1024 states needs more than 2^30 bytes of lattice (4 bytes a frame and state):
    FDNN_E_ARG from the plan, before any launch, nothing allocated; forward only needs no lattice and is not refused for it."""
    import torch

    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    L, i32, i64 = api.lib(), api.C.POINTER(api.C.c_int), api.C.POINTER(api.C.c_longlong)
    cap_words = api.fb_limits()["scratch_cap_mib"] * (1 << 20) // 4
    assert api.fb_scratch_words([1 << 18], [0, 1024]) == cap_words
    with pytest.raises(api.FdnnError):
        api.fb_scratch_words([(1 << 18) + 1], [0, 1024])
    before = api.fb_launches()
    ap = np.zeros(1025, np.int32)

    def call(T, scratch=0, words=0):
        a = [np.array(v, t) for v, t in (([T], np.int32), ([0], np.int64), ([8], np.int32), ([0, 1024], np.int32))]
        rc = L.fdnn_fb_rows_device(None, p, a[0].ctypes.data_as(i32), a[1].ctypes.data_as(i64), a[2].ctypes.data_as(i32), a[3].ctypes.data_as(i32),
                                   ap.ctypes.data_as(i32), ap.ctypes.data_as(i32), 1, p, None, p, None, None, None, None, p, None, None, scratch, words, p, p, None)
        return rc, L.fdnn_last_error().decode(errors="replace")

    rc, msg = call((1 << 18) + 1, p, 1 << 40)  # (however much scratch the caller claims to bring)
    assert rc == api.FDNN_E_ARG and "above" in msg and str(1 << 30) in msg, msg
    rc, msg = call(1 << 18)  # passes the cap: the refusal is the missing scratch
    assert rc == api.FDNN_E_ARG and "fdnn_fb_scratch_words" in msg and str(cap_words) in msg, msg
    torch.cuda.synchronize()
    assert api.fb_launches() == before
