"""The frames form of the best path through the model, on the `tiny` net and the signal net k48 (tests/signal_nets.py): every
entry point returns the host restatement's bytes (api.align_frames_ref) over the rows that fdnn_calculate_lazy_sets returns for
the graphs' node sets, turned into scores by api.loglik_entries_ref; consequences (a) and (e) hold against alignGraph."""
import numpy as np
import pytest

import align_cases as AC
import align_graph_cases as GC
import loglik_cases as LL
import signal_nets as SN
from fast_dnn_amd import api, convert, formats as F

pytestmark = pytest.mark.gpu
HANDLES = ((-20.0, api.LOGLIK_F32), (-20.0, api.LOGLIK_F16))
KALDI = (list(range(-5, 6)), 39)


def same(got, want):
    flat = lambda r: (r[0].view(np.uint32), r[1], r[2], r[3][0].view(np.uint32), r[3][1])
    return all(np.array_equal(g, w) for g, w in zip(flat(got), flat(want)))


@pytest.mark.parametrize("net", ("tiny", "k48"))
def test_every_entry_point_and_the_consequences_on_the_device(net, tiny_model_path, tmp_models):
    import torch

    dnn = api.QuantizedDnn.loadFromFile(tiny_model_path if net == "tiny" else SN.path("k48", "gauss", tmp_models))
    x, n_segs = (F.synth_features(33, 432, seed=2504), 1) if net == "tiny" else (SN.features("k48"), 2)
    dense = dnn.calculate(x)
    n, O = dense.shape
    seg_rows = AC.seg_rows_of(n, n_segs)
    graphs = GC.silence_graphs(dense, seg_rows, 31)
    packed = api.pack_graphs(graphs)
    states, lp, base = int(packed["statePtr"][-1]), LL.priors(O), [5000 * (s + 1) for s in range(n_segs)]
    # keywords for (e): every loop at -30, more than a frame's score makes up for, so the best path is short and begins late
    loops = [np.asarray(g["arc_src"]) == np.repeat(np.arange(len(g["states"])), np.diff(g["arc_ptr"])) for g in graphs]
    keywords = [dict(g, arc_lp=np.where(l, np.float32(-30.0), g["arc_lp"]).astype(np.float32)) for g, l in zip(graphs, loops)]
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutput(x)
    rng = np.random.default_rng(3)
    carry = (rng.uniform(-30, -5, states).astype(np.float32), rng.integers(-50, 50, states).astype(np.int32))
    for handle in HANDLES:
        ll = api.Loglik(lp, *handle)
        e, T, off, ln, col = GC.composed(dnn, x, lp, handle, seg_rows, packed)[1]
        for free, cin in ((False, None), (True, carry)):
            want = api.align_frames_ref(e, T, off, ln, packed, col, free_start=free, frame_base=base, carry=cin)
            assert not np.isnan(want[0]).any() and np.isfinite(want[0]).mean() > 0.5
            assert same(dnn.calculateAlignFrames(x, ll, seg_rows, packed, free, base, cin), want), (net, handle, free)
            assert same(ctx.alignFrames(ll, seg_rows, packed, free, base, cin), want), (net, handle, free)
            outs = [torch.full((size,), -7, dtype=ty, device="cuda") for size, ty in ((n, torch.float32), (n, torch.int32), (n, torch.int32),
                                                                                     (states, torch.float32), (states, torch.int32))]
            keep = [torch.from_numpy(a).cuda() for a in cin or ()]
            st = torch.cuda.Stream()
            torch.cuda.synchronize()
            ctx.alignFramesDevice(ll, seg_rows, packed, *[o.data_ptr() for o in outs[:3]], free, base, *([k.data_ptr() for k in keep] or [0, 0]), outs[3].data_ptr(), outs[4].data_ptr(), st.cuda_stream)
            st.synchronize()
            got = [o.cpu().numpy() for o in outs]
            assert same((got[0], got[1], got[2], (got[3], got[4])), want)
        anchored, free = ctx.alignFrames(ll, seg_rows, packed, False, base), ctx.alignFrames(ll, seg_rows, api.pack_graphs(keywords), True, base)
        late = 0
        for s in range(n_segs):
            a, b = int(seg_rows[s]), int(seg_rows[s + 1])
            one, kw = api.pack_graphs(graphs[s:s + 1]), api.pack_graphs(keywords[s:s + 1])
            for t in range(a, b, 3):
                path, total = ctx.alignGraph(ll, [a, t + 1], one)  # (a): the prefix's total, and where it is finite its last state
                assert total.view(np.uint32)[0] == anchored[0].view(np.uint32)[t] and (not np.isfinite(total[0]) or (anchored[1][t], anchored[2][t]) == (path[-1], base[s]))
                if np.isfinite(free[0][t]):  # (e): the reported span's total and last state
                    begin = a + int(free[2][t]) - base[s]
                    path, total = ctx.alignGraph(ll, [begin, t + 1], kw)
                    assert a <= begin <= t and total.view(np.uint32)[0] == free[0].view(np.uint32)[t] and path[-1] == free[1][t], (net, s, t)
                    late += begin > a
        assert late > 0  # not blind
        ll.delete()
    ctx.delete()
    dnn.delete()


def test_raw_frames_and_a_chunked_call(mid_model_path):
    dnn = api.QuantizedDnn.loadFromFile(mid_model_path)
    O = dnn.calculate(F.synth_features(2, 432, seed=1)).shape[1]
    ll = api.Loglik(LL.priors(O), -20.0, api.LOGLIK_F16)
    rng = np.random.default_rng(44)
    graphs = []
    for n_words in (8, 12, 6):
        g = api.optional_silence_graph([rng.integers(1, O, 4).tolist() for _ in range(n_words)], 0)
        graphs.append(dict(g, arc_lp=np.log(rng.uniform(0.05, 0.95, g["arc_lp"].size)).astype(np.float32)))
    packed = api.pack_graphs(graphs)
    # raw frames, every segment an utterance of its own, equal the spliced rows
    dnn.setSplice(*KALDI)
    raw = (rng.standard_normal((150, 39)) * 3).astype(np.float32)
    seg_rows = np.array([0, 50, 110, 150], np.int32)
    x = np.concatenate([convert.splice_frames(raw[a:b], KALDI[0], 432) for a, b in zip(seg_rows[:-1], seg_rows[1:])])
    got = dnn.calculateAlignFramesRaw(raw, ll, seg_rows, packed, True, [7, 9, 11])
    assert np.isfinite(got[0]).any() and same(got, dnn.calculateAlignFrames(x, ll, seg_rows, packed, True, [7, 9, 11]))
    dnn.setSplice([], 0)
    # two chunks that cut the middle segment give that segment's one-chunk bytes
    n = 20480 + 300
    cut = api.frame_chunks(n, True)[1][0]
    assert len(api.frame_chunks(n, True)) == 2
    seg_rows = np.array([0, cut - 80, cut + 120, n], np.int32)
    x = F.synth_features(n, 432, seed=2600)
    got = dnn.calculateAlignFrames(x, ll, seg_rows, packed, True, [1, 2, 3])
    a, b, sp = int(seg_rows[1]), int(seg_rows[2]), packed["statePtr"]
    alone = dnn.calculateAlignFrames(x[a:b], ll, [0, b - a], api.pack_graphs(graphs[1:2]), True, [2])
    assert same((got[0][a:b], got[1][a:b], got[2][a:b], (got[3][0][sp[1]:sp[2]], got[3][1][sp[1]:sp[2]])), alone) and np.isfinite(alone[0][-1])
    ll.delete()
    dnn.delete()
