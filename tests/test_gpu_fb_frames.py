"""The frames form of the summed alignment graphs through the model (fdnn_calculate_fb_frames and its raw-frame, context and
device forms), on the nets of tests/test_gpu_fb.py: every entry point's frame_total and alpha_out are the host restatement's
(api.fb_frames_ref, held to float64 by tests/test_fb_frames_host.py) over the bytes that fdnn_calculate_lazy_sets returns for
the graphs' node sets, turned into scores by api.loglik_entries_ref -- the lazy path is untouched, so the composition is exact."""
import numpy as np
import pytest

import align_graph_cases as GC
import loglik_cases as LL
from fast_dnn_amd import api, convert, formats as F
from test_gpu_fb import HANDLES, KALDI, NETS, SIL, fixtures, nets, seg_rows_of  # noqa: F401 (fixtures and nets are pytest fixtures)

pytestmark = pytest.mark.gpu


def same(got, want):
    return all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want))


def composed(dnn, x, lp, handle, seg_rows, packed, **kw):
    """The restatement over the lazy sets call's bytes -> (frame_total, alpha_out)."""
    _, (e, T, off, ln, col) = GC.composed(dnn, x, lp, handle, seg_rows, packed)
    return api.fb_frames_ref(e, T, off, ln, packed, col, **kw)


@pytest.mark.parametrize("net", list(NETS))
def test_every_entry_point_returns_the_restatements_bytes(nets, net):
    import torch

    dnn, x, dense = nets(net)
    n, O = dense.shape
    seg_rows = seg_rows_of(n, NETS[net][1])
    packed = api.pack_graphs(GC.silence_graphs(dense, seg_rows, 31))
    states = int(packed["statePtr"][-1])
    lp = LL.priors(O)
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutput(x)
    st = torch.cuda.Stream()
    carry = np.random.default_rng(3).uniform(-30, -5, states).astype(np.float32)
    for handle in HANDLES:
        ll = api.Loglik(lp, *handle)
        for free, alpha_in in ((False, None), (True, None), (True, carry)):
            want = composed(dnn, x, lp, handle, seg_rows, packed, free_start=free, alpha_in=alpha_in)
            assert not np.isnan(want[0]).any() and np.isfinite(want[0]).mean() > 0.5
            before = api.fb_frames_launches(), api.fb_launches()
            assert same(dnn.calculateFbFrames(x, ll, seg_rows, packed, free, alpha_in), want), (net, handle, free)
            assert api.fb_frames_launches()[2] == before[0][2] + 1 and api.fb_launches() == before[1]  # a counter of their own
            assert same(ctx.fbFrames(ll, seg_rows, packed, free, alpha_in), want), (net, handle, free)
            for mode in (1, 2):
                api.set_fb_kernel(mode)
                try:
                    assert same(ctx.fbFrames(ll, seg_rows, packed, free, alpha_in), want), (net, handle, free, mode)
                finally:
                    api.set_fb_kernel(0)
            d_tot = torch.full((n + 8,), -7.0, dtype=torch.float32, device="cuda")
            d_out = torch.full((states + 8,), -7.0, dtype=torch.float32, device="cuda")
            d_in = torch.from_numpy(alpha_in).cuda() if alpha_in is not None else None
            torch.cuda.synchronize()
            ctx.fbFramesDevice(ll, seg_rows, packed, d_tot.data_ptr() + 16, free, d_in.data_ptr() if d_in is not None else 0, d_out.data_ptr() + 16, st.cuda_stream)
            st.synchronize()
            t, o = d_tot.cpu().numpy(), d_out.cpu().numpy()
            assert (t[:4] == -7).all() and (t[-4:] == -7).all() and (o[:4] == -7).all() and (o[-4:] == -7).all() and same((t[4:-4], o[4:-4]), want)
        # (a): anchored, the last frame of every segment is fdnn_calculate_fb's total, as bits
        anchored = dnn.calculateFbFrames(x, ll, seg_rows, packed)[0]
        total = dnn.calculateForwardBackward(x, ll, seg_rows, packed, want_gamma=False)[0]
        assert np.array_equal(anchored[seg_rows[1:] - 1].view(np.uint32), total.view(np.uint32))
        # (b): the context's rows pushed in two calls with carry are the one call's bytes
        one = api.pack_graphs(GC.silence_graphs(dense, np.array([0, n]), 32))
        whole = ctx.fbFrames(ll, [0, n], one, True)
        a = ctx.fbFrames(ll, [0, n // 3], one, True)
        b = ctx.fbFrames(ll, [n // 3, n], one, True, a[1])
        assert same((np.concatenate([a[0], b[0]]), b[1]), whole)
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
        got = dnn.calculateFbFramesRaw(raw, ll, seg_rows, packed, True)
        assert np.isfinite(got[0]).mean() > 0.5 and same(got, dnn.calculateFbFrames(x, ll, seg_rows, packed, True))
        ll.delete()
    finally:
        dnn.setSplice([], 0)


def test_two_chunks_that_cut_a_segment_give_the_uncut_bytes(nets):
    dnn, _, dense = nets("mid")
    n = 20480 + 300
    cut = api.frame_chunks(n, True)[1][0]
    assert len(api.frame_chunks(n, True)) == 2 and len(api.frame_chunks(n, False)) == 2
    seg_rows = np.array([0, cut - 80, cut + 120, n], np.int32)  # the middle segment is cut by the chunk
    x = F.synth_features(n, 432, seed=2600)
    rng = np.random.default_rng(44)
    graphs = []
    for n_words in (8, 12, 6):
        g = api.optional_silence_graph([rng.integers(1, dense.shape[1], 4).tolist() for _ in range(n_words)], SIL)
        g["arc_lp"] = np.log(rng.uniform(0.05, 0.95, g["arc_lp"].size)).astype(np.float32)
        graphs.append(g)
    packed = api.pack_graphs(graphs)
    ll = api.Loglik(LL.priors(dense.shape[1]), -20.0, api.LOGLIK_F16)
    before = api.fb_frames_launches()
    got = dnn.calculateFbFrames(x, ll, seg_rows, packed, True)
    delta = tuple(b - a for a, b in zip(before, api.fb_frames_launches()))
    assert delta[0] + delta[1] == delta[2] == 1  # the sweep and the row totals run ONCE, behind the last chunk
    a, b = int(seg_rows[1]), int(seg_rows[2])
    alone = dnn.calculateFbFrames(x[a:b], ll, [0, b - a], api.pack_graphs(graphs[1:2]), True)  # one chunk
    sp = packed["statePtr"]
    assert same((got[0][a:b], got[1][sp[1]:sp[2]]), alone) and np.isfinite(alone[0][-1])
    ll.delete()


def test_the_carry_row_in_place_through_the_context(nets):
    """fbFramesDevice with d_alpha_out == d_alpha_in, ONE buffer (fdnn.h: allowed): a stream's second call gives the
    two-buffer call's frame_total and carry row byte for byte -- which are the uncut call's --, anchored and free, in both
    forced forms, on a side stream."""
    import torch

    dnn, x, dense = nets("tiny")
    n, O = dense.shape
    one = api.pack_graphs(GC.silence_graphs(dense, np.array([0, n]), 35))
    S, cut = int(one["statePtr"][-1]), n // 2
    ll = api.Loglik(LL.priors(O), -20.0, api.LOGLIK_F16)
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutput(x)
    st = torch.cuda.Stream()
    try:
        for free in (False, True):
            whole = ctx.fbFrames(ll, [0, n], one, free)
            assert not np.isnan(whole[0]).any() and np.isfinite(whole[0][-1])
            for mode in (1, 2):
                api.set_fb_kernel(mode)
                outs = []
                for in_place in (False, True):
                    d_tot = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
                    d_a = torch.full((S,), -7.0, dtype=torch.float32, device="cuda")
                    d_b = d_a if in_place else torch.full((S,), -7.0, dtype=torch.float32, device="cuda")
                    torch.cuda.synchronize()
                    ctx.fbFramesDevice(ll, [0, cut], one, d_tot.data_ptr(), free, 0, d_a.data_ptr(), st.cuda_stream)
                    ctx.fbFramesDevice(ll, [cut, n], one, d_tot.data_ptr() + 4 * cut, free, d_a.data_ptr(), d_b.data_ptr(), st.cuda_stream)
                    st.synchronize()
                    outs.append((d_tot.cpu().numpy(), d_b.cpu().numpy()))
                assert same(outs[1], outs[0]) and same(outs[1], whole), (free, mode)
    finally:
        api.set_fb_kernel(0)
        ll.delete()
        ctx.delete()
