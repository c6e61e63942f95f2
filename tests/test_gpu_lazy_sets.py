"""Lazy output for per-segment node sets (fdnn_ctx_lazy_output_sets / _device, fdnn_calculate_lazy_sets; fdnn_sets.hip) with
the MFMA kernel forced (fdnn_debug_set_kernel(1)).  Every segment is rows [a, b) of a tests/lazy_set_cases.py case with
that case's set, so what it must return is rows [a, b) of SC.reference: the int32 accumulators bit for bit, probabilities
and inactive values within 2e-6 (SC.TIGHT) -- tests/test_lazy_set_host.py shows that the normative sum order meets that bar on
exactly these (row, set) pairs.  And the byte contract: a row's bytes are those of fdnn_ctx_lazy_output_set on its segment
alone and of fdnn_ctx_lazy_output_lists with the sets repeated per row, whatever the entry point, the segmentation or the
launch a segment falls into -- with ONE launch of the MFMA kernel for up to 64 segments."""
import numpy as np
import pytest

import lazy_lists_cases as LC
import lazy_set_cases as SC
import softmax_ref as SR
from fast_dnn_amd import api, formats as F

pytestmark = pytest.mark.gpu
TIGHT = SC.TIGHT


@pytest.fixture(scope="module")
def fixtures(mid_model_path, sat_model_path, tiny_model_path, net_model_path):
    api.set_kernel(1)
    yield {"mid": mid_model_path, "sat": sat_model_path, "tiny": tiny_model_path, "full": net_model_path}
    api.set_kernel(0)
    SC.release()
    for d in _MODELS.values():
        d.delete()
    _MODELS.clear()


_MODELS = {}


def model(net, fixtures):
    if net not in _MODELS:
        _MODELS[net] = api.QuantizedDnn.loadFromFile(LC.model_path(net, fixtures))
    return _MODELS[net]


def same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Composition:
    """segments: [(rows, case name)] from row `first` on; the tables of the call and, from SC.reference alone, what it must
    return (flat, ragged like probs)."""

    def __init__(self, segments, fixtures, first=0, row_of=None):
        self.segments = segments
        self.refs = [SC.reference(name, fixtures) for _, name in segments]
        self.sets = [r["nodes"] for r in self.refs]
        self.seg_rows = np.cumsum([first] + [rows for rows, _ in segments]).astype(np.int32)
        self.set_ptr = np.cumsum([0] + [nd.size for nd in self.sets]).astype(np.int32)
        self.nodes = np.concatenate(self.sets + [np.zeros(0, np.int32)]).astype(np.int32)
        self.rows = int(self.seg_rows[-1] - self.seg_rows[0])
        row_of = row_of or (lambda r: r)  # context row -> row of the case's reference
        src = [[row_of(r) for r in range(a, b)] for a, b in zip(self.seg_rows[:-1], self.seg_rows[1:])]
        self.want_acc = np.concatenate([r["acc"][s].ravel() for r, s in zip(self.refs, src)] + [np.zeros(0, np.int32)])
        self.want_probs = np.concatenate([r["want_probs"][s].ravel() for r, s in zip(self.refs, src)] + [np.zeros(0, np.float32)])
        self.want_inactive = np.concatenate([r["want_inactive"][s] for r, s in zip(self.refs, src)] + [np.zeros(0, np.float32)])
        self.nnz = self.want_probs.size
        self.x = self.refs[0]["x"]

    def tables(self):
        return self.seg_rows, self.set_ptr, self.nodes

    def blocks(self, flat):
        """the flat probs as one [rows][len] array per segment"""
        out, off = [], 0
        for (rows, _), nd in zip(self.segments, self.sets):
            out.append(flat[off:off + rows * nd.size].reshape(rows, nd.size))
            off += rows * nd.size
        assert off == flat.size
        return out


def device_form(dnn, x, calls):
    """forward_hidden_device and one sets call per entry of `calls` (tables) on ONE non-default stream, no synchronisation
    between them, sentinels past probs and inactive -> [(probs flat, inactive)]"""
    import torch

    st = torch.cuda.Stream()
    dx = torch.from_numpy(x).cuda()
    bufs = []
    for seg_rows, set_ptr, nodes in calls:
        rows = int(seg_rows[-1] - seg_rows[0])
        nnz = int((np.diff(seg_rows.astype(np.int64)) * np.diff(set_ptr.astype(np.int64))).sum())
        bufs.append((torch.from_numpy(np.concatenate((nodes, np.zeros(1, np.int32)))).cuda(),
                     torch.full((nnz + 1,), -7.0, dtype=torch.float32, device="cuda"),
                     torch.full((rows + 1,), -7.0, dtype=torch.float32, device="cuda"), nnz, rows))
    torch.cuda.synchronize()
    ctx = dnn.getNewLazyContext(x.shape[0])
    ctx.calculateUntilOutputDevice(dx.data_ptr(), st.cuda_stream)
    for (seg_rows, set_ptr, _), b in zip(calls, bufs):
        ctx.calculateForOutputNodeSetsDevice(seg_rows, set_ptr, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), st.cuda_stream)
    st.synchronize()
    ctx.delete()
    out = []
    for dnd, dp, di, nnz, rows in bufs:
        probs, inactive = dp.cpu().numpy(), di.cpu().numpy()
        assert probs[nnz] == -7.0 and inactive[rows] == -7.0  # nothing written past the results
        out.append((probs[:nnz], inactive[:rows]))
    return out


def against_the_oracle(comp, ctx, probs, inactive):
    """accumulators bit for bit, probs and inactive within TIGHT, the bytes of the set path per segment and of the list path"""
    acc = ctx.setsAccumulators(*comp.tables())
    assert np.array_equal(acc, comp.want_acc), f"{int((acc != comp.want_acc).sum())} accumulators differ from the oracle"
    worst = np.abs(probs - comp.want_probs).max(initial=0.0)
    print(f"\n[sets] {[(r, n) for r, n in comp.segments]}: max |p - oracle| {worst:.3e}", flush=True)
    assert probs.shape == (comp.nnz,) and worst <= TIGHT
    known = ~np.isnan(comp.want_inactive)
    assert inactive.shape == (comp.rows,) and np.abs(inactive[known] - comp.want_inactive[known]).max(initial=0.0) <= TIGHT
    for s, block in enumerate(comp.blocks(probs)):
        a, b = int(comp.seg_rows[s]), int(comp.seg_rows[s + 1])
        sp, si = ctx.calculateForOutputNodeSet(comp.sets[s], a, b - a)
        assert same_bytes(sp, block) and same_bytes(si, inactive[a - comp.seg_rows[0]:b - comp.seg_rows[0]]), f"segment {s}"
    row_ptr, list_nodes = F.sets_to_lists(*comp.tables())
    lp, li = ctx.calculateForOutputNodesLists(row_ptr, list_nodes, first=int(comp.seg_rows[0]))
    assert same_bytes(lp, probs) and same_bytes(li, inactive)


MID_EDGES = [(1, "mid.len65"), (31, "mid.len0"), (0, "mid.len1"), (33, "mid.len129"), (35, "mid.len64")]


def test_one_composition_with_every_edge_in_one_launch(fixtures):
    """Segment boundaries at rows 1, 32 and 65: the next segment's rows share what would be a 32-frame tile (1 | 31) and
    straddle tiles (33, 35); an empty segment, a zero-length set, sets of 1, 2 and 3 node tiles.  One MFMA launch serves the
    whole call -- and none of fdnn_set.hip's."""
    comp = Composition(MID_EDGES, fixtures)
    dnn = model("mid", fixtures)
    assert comp.rows == 100 and comp.seg_rows.tolist() == [0, 1, 32, 32, 65, 100]
    ctx = dnn.getNewLazyContext(100)
    ctx.calculateUntilOutput(comp.x)
    tb, sb, lb = api.sets_launches(), api.set_launches(), api.lists_launches()
    probs, inactive = ctx.calculateForOutputNodeSets(*comp.tables())
    ta, sa, la = api.sets_launches(), api.set_launches(), api.lists_launches()
    assert ta[1] == tb[1] + 1 and ta[0] == tb[0] and ta[2] == tb[2]  # exactly ONE launch of the MFMA kernel (mid has pairs: the walk)
    assert sa == sb                                                   # ... and none counted for fdnn_set.hip
    assert la[0] == lb[0] and la[1] == lb[1] and la[2] == lb[2] + 1   # of the list kernels only the finish pass, once
    against_the_oracle(comp, ctx, probs, inactive)
    assert (inactive[1:32] == np.float32(1.0) / np.float32(1000)).all()  # the zero-length set: 1 / O
    # the forced fallback: the same bytes, no MFMA launch
    api.set_kernel(2)
    try:
        tb = api.sets_launches()
        fp, fi = ctx.calculateForOutputNodeSets(*comp.tables())
        ta = api.sets_launches()
        assert np.array_equal(ctx.setsAccumulators(*comp.tables()), comp.want_acc)
    finally:
        api.set_kernel(1)
    assert same_bytes(fp, probs) and same_bytes(fi, inactive)
    assert ta[:2] == tb[:2] and ta[2] == tb[2] + 1
    ctx.delete()
    # the device form (sentinels past probs and inactive intact) and the one-call form
    tb = api.sets_launches()
    (dp, di), = device_form(dnn, comp.x, [comp.tables()])
    assert api.sets_launches()[1] == tb[1] + 1
    assert same_bytes(dp, probs) and same_bytes(di, inactive)
    op, oi = dnn.calculateLazySets(comp.x, *comp.tables())
    assert same_bytes(op, probs) and same_bytes(oi, inactive)
    # no segment is a no-op, in every form
    ctx = dnn.getNewLazyContext(100)
    ctx.calculateUntilOutput(comp.x)
    p0, i0 = ctx.calculateForOutputNodeSets([5], [0], [])
    assert p0.size == 0 and i0.size == 0
    ctx.delete()


def test_one_call_form_in_chunks_cuts_a_segment(fixtures, mid_model_path):
    """fdnn_calculate_lazy_sets over 21 000 frames runs as chunks of 20 480 + 520 (fdnn::frame_chunks): the middle segment
    (rows 7 000 .. 20 499) is cut in two and keeps its set.  The bytes of fdnn_calculate_lazy_set per segment, and the oracle's
    lazy rows around every boundary."""
    from oracle.oracle import Oracle

    n, O = 21000, 1000
    dnn = model("mid", fixtures)
    x = F.synth_features(n, 432, seed=78)
    sets = [SC.reference(name, fixtures)["nodes"] for name in ("mid.len1", "mid.len65", "mid.len129")]
    seg_rows = np.array([0, 7000, 20500, n], np.int32)
    set_ptr = np.cumsum([0] + [nd.size for nd in sets]).astype(np.int32)
    tb = api.sets_launches()
    probs, inactive = dnn.calculateLazySets(x, seg_rows, set_ptr, np.concatenate(sets))
    ta = api.sets_launches()
    assert ta[1] == tb[1] + 2 and ta[0] == tb[0] and ta[2] == tb[2]  # one launch per chunk
    off = 0
    for s, nd in enumerate(sets):
        a, b = int(seg_rows[s]), int(seg_rows[s + 1])
        sp, si = dnn.calculateLazySet(x[a:b], nd)
        assert same_bytes(probs[off:off + (b - a) * nd.size].reshape(b - a, nd.size), sp) and same_bytes(inactive[a:b], si), s
        off += (b - a) * nd.size
    assert off == probs.size
    idx = np.array([0, 6999, 7000, 20479, 20480, 20499, 20500, n - 1])
    masks = np.zeros((idx.size, O), np.int8)
    for k, r in enumerate(idx):
        masks[k, sets[int(np.searchsorted(seg_rows, r, side="right")) - 1]] = 1
    want = Oracle(mid_model_path).lazy(x[idx], masks)
    row_ptr, list_nodes = F.sets_to_lists(seg_rows, set_ptr, np.concatenate(sets))
    for k, r in enumerate(idx):
        got = np.full(O, inactive[r], np.float32)
        got[list_nodes[row_ptr[r]:row_ptr[r + 1]]] = probs[row_ptr[r]:row_ptr[r + 1]]
        assert np.abs(got - want[k]).max() <= TIGHT, r


def test_another_segmentation_and_order_give_the_same_bytes(fixtures):
    """Bytes per (row, set): the same pairs cut into other segments, and a set in another segment position, against the set
    scored over the whole context."""
    X, Y = "mid.len65", "mid.len129"
    dnn = model("mid", fixtures)
    a = Composition([(50, X), (50, Y)], fixtures)
    b = Composition([(7, X), (43, X), (14, Y), (36, Y)], fixtures)
    c = Composition([(50, Y), (50, X)], fixtures)
    d = Composition([(33, Y), (17, Y), (1, X), (49, X)], fixtures)
    ctx = dnn.getNewLazyContext(100)
    ctx.calculateUntilOutput(a.x)
    got = {k: ctx.calculateForOutputNodeSets(*comp.tables()) for k, comp in (("a", a), ("b", b), ("c", c), ("d", d))}
    for k, comp in (("a", a), ("b", b), ("c", c), ("d", d)):
        assert np.abs(got[k][0] - comp.want_probs).max() <= TIGHT and np.abs(got[k][1] - comp.want_inactive).max() <= TIGHT
    assert same_bytes(got["a"][0], got["b"][0]) and same_bytes(got["a"][1], got["b"][1])  # (blocks of one set are adjacent)
    assert same_bytes(got["c"][0], got["d"][0]) and same_bytes(got["c"][1], got["d"][1])
    whole = {name: ctx.calculateForOutputNodeSet(SC.reference(name, fixtures)["nodes"]) for name in (X, Y)}
    ctx.delete()
    ax, ay = a.blocks(got["a"][0])
    cy, cx = c.blocks(got["c"][0])
    assert same_bytes(ax, whole[X][0][:50]) and same_bytes(ay, whole[Y][0][50:]) and same_bytes(cy, whole[Y][0][:50]) and same_bytes(cx, whole[X][0][50:])
    assert same_bytes(got["a"][1], np.concatenate((whole[X][1][:50], whole[Y][1][50:])))
    assert same_bytes(got["c"][1], np.concatenate((whole[Y][1][:50], whole[X][1][50:])))
    # a call that begins above row 0
    e = Composition([(20, Y), (13, X)], fixtures, first=37)
    ctx = dnn.getNewLazyContext(100)
    ctx.calculateUntilOutput(e.x)
    probs, inactive = ctx.calculateForOutputNodeSets(*e.tables())
    ctx.delete()
    ey, ex = e.blocks(probs)
    assert same_bytes(ey, whole[Y][0][37:57]) and same_bytes(ex, whole[X][0][57:70])
    assert same_bytes(inactive, np.concatenate((whole[Y][1][37:57], whole[X][1][57:70])))


def test_130_one_row_segments_cross_the_64_segment_cut(fixtures):
    """130 one-row segments (the mid fixture's 100 rows, the first 30 repeated): ceil(130 / 64) = 3 launches, the same bytes."""
    names = ["mid.len65", "mid.len0", "mid.len1", "mid.len129", "mid.len64"]
    comp = Composition([(1, names[s % 5]) for s in range(130)], fixtures, row_of=lambda r: r % 100)
    dnn = model("mid", fixtures)
    x = np.concatenate((comp.x, comp.x[:30]))
    ctx = dnn.getNewLazyContext(130)
    ctx.calculateUntilOutput(x)
    tb, sb = api.sets_launches(), api.set_launches()
    probs, inactive = ctx.calculateForOutputNodeSets(*comp.tables())
    ta, sa = api.sets_launches(), api.set_launches()
    assert ta[1] == tb[1] + 3 and ta[0] == tb[0] and ta[2] == tb[2] and sa == sb
    against_the_oracle(comp, ctx, probs, inactive)
    ctx.delete()
    (dp, di), = device_form(dnn, x, [comp.tables()])
    assert same_bytes(dp, probs) and same_bytes(di, inactive)


@pytest.mark.parametrize("net,n,segments,counter", [
    ("sat", 33, [(16, "sat.len10"), (17, "sat.len200")], 1),                                   # the walk instance
    ("n256/256/nosat", 33, [(16, "nosat.len100"), (17, "nosat.len100")], 0),                   # the walk-free instance
    ("full", 64, [(20, "full.len8"), (24, "full.len80"), (20, "full.len8000")], 1),            # K = 2048, the longest chain
])
def test_other_nets(fixtures, net, n, segments, counter):
    comp = Composition(segments, fixtures)
    dnn = model(net, fixtures)
    assert comp.rows == n
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutput(comp.x)
    tb = api.sets_launches()
    probs, inactive = ctx.calculateForOutputNodeSets(*comp.tables())
    ta = api.sets_launches()
    assert ta[counter] == tb[counter] + 1 and ta[1 - counter] == tb[1 - counter] and ta[2] == tb[2]
    against_the_oracle(comp, ctx, probs, inactive)
    ctx.delete()
    op, oi = dnn.calculateLazySets(comp.x, *comp.tables())
    assert same_bytes(op, probs) and same_bytes(oi, inactive)


def test_a_layer_the_kernel_does_not_stage_goes_to_the_list_kernels(fixtures):
    """K = 2304: under the default rule and with the MFMA kernel 'forced' the list kernels serve the call."""
    comp = Composition([(16, "k2304.len70"), (17, "k2304.len70")], fixtures)
    dnn = model("k2304", fixtures)
    ctx = dnn.getNewLazyContext(33)
    ctx.calculateUntilOutput(comp.x)
    results = []
    try:
        for mode in (0, 1):
            api.set_kernel(mode)
            tb = api.sets_launches()
            results.append(ctx.calculateForOutputNodeSets(*comp.tables()))
            ta = api.sets_launches()
            assert ta[:2] == tb[:2] and ta[2] == tb[2] + 1
    finally:
        api.set_kernel(1)
    assert same_bytes(results[0][0], results[1][0]) and same_bytes(results[0][1], results[1][1])
    against_the_oracle(comp, ctx, *results[1])
    ctx.delete()


def test_the_overflowing_logits_stay_in_their_segment(fixtures):
    """tail/ovf, one hot and one cold segment: the oracle's NaN / 0 pattern in the hot segment only."""
    comp = Composition([(16, "tail.ovf.hot"), (17, "tail.ovf.cold")], fixtures)
    dnn = model("tail/ovf", fixtures)
    probs, inactive = dnn.calculateLazySets(comp.x, *comp.tables())
    row_ptr, list_nodes = F.sets_to_lists(*comp.tables())
    got = F.lists_to_rows(row_ptr, list_nodes, probs, inactive, 256)
    hot, cold = comp.refs
    assert np.array_equal(got[:16], hot["want_rows"][:16], equal_nan=True)  # four NaN, every other entry 0, inactive 0
    assert (np.isnan(got[:16]).sum(1) == 4).all() and (inactive[:16] == 0).all()
    assert np.isfinite(got[16:]).all() and np.abs(got[16:] - cold["want_rows"][16:]).max() <= TIGHT


def test_relative_bound_on_the_ladder_net(fixtures):
    """rel.lad256.len100 and rel.lad256.full as two segments: every element within lazy_lists_cases.relative_bound of float64."""
    comp = Composition([(16, "rel.lad256.len100"), (17, "rel.lad256.full")], fixtures)
    dnn = model("lad/256", fixtures)
    tb = api.sets_launches()
    probs, inactive = dnn.calculateLazySets(comp.x, *comp.tables())
    ta = api.sets_launches()
    assert sum(ta[:2]) == sum(tb[:2]) + 1 and ta[2] == tb[2]
    row_ptr, list_nodes = F.sets_to_lists(*comp.tables())
    got = F.lists_to_rows(row_ptr, list_nodes, probs, inactive, 256)
    assert not np.isnan(got).any()
    worst_ratio = 0.0
    for f in range(33):
        r = comp.refs[0 if f < 16 else 1]
        z = r["z"][f]
        p64 = SR.softmax64(r["z"][f:f + 1])[0]
        assert (p64 >= SR.TINY).all()
        b = LC.relative_bound(z, r["masks"][f] != 0, p64)
        rel = np.abs(got[f].astype(np.float64) / p64 - 1.0)
        worst_ratio = max(worst_ratio, float((rel / b).max()))
        assert (rel <= b).all(), f"row {f}: worst rel / bound {float((rel / b).max()):.3f}"
    print(f"\n[sets-range] lad/256: worst_rel_over_bound {worst_ratio:.3f}", flush=True)


@pytest.mark.parametrize("bad", [1000, -1])
def test_device_sets_with_a_node_outside_the_layer(fixtures, bad):
    """The device form does not validate the sets: node O or node -1 in the MIDDLE segment's set makes that segment's
    probs and inactive values NaN and no other's; the next valid call on the context is correct."""
    comp = Composition([(33, "mid.len65"), (30, "mid.len129"), (37, "mid.len64")], fixtures)
    dnn = model("mid", fixtures)
    seg_rows, set_ptr, nodes = comp.tables()
    wrong = nodes.copy()
    wrong[set_ptr[1] + 70] = bad
    (p, i), (gp, gi) = device_form(dnn, comp.x, [(seg_rows, set_ptr, wrong), comp.tables()])
    first, middle, last = comp.blocks(p)
    want = comp.blocks(comp.want_probs)
    assert np.isnan(middle).all() and np.isnan(i[33:63]).all()
    assert np.abs(first - want[0]).max() <= TIGHT and np.abs(last - want[2]).max() <= TIGHT
    assert np.abs(i[:33] - comp.want_inactive[:33]).max() <= TIGHT and np.abs(i[63:] - comp.want_inactive[63:]).max() <= TIGHT
    assert np.abs(gp - comp.want_probs).max() <= TIGHT and np.abs(gi - comp.want_inactive).max() <= TIGHT
    assert same_bytes(first, comp.blocks(gp)[0]) and same_bytes(last, comp.blocks(gp)[2])


def test_errors(fixtures):
    comp = Composition(MID_EDGES, fixtures)
    dnn = model("mid", fixtures)
    ctx = dnn.getNewLazyContext(100)
    with pytest.raises(api.FdnnError) as e:
        ctx.calculateForOutputNodeSets([0, 10], [0, 2], [1, 2])  # before the hidden layers
    assert e.value.code == api.FDNN_E_STATE
    with pytest.raises(api.FdnnError) as e:
        ctx.calculateForOutputNodeSetsDevice([0, 10], [0, 2], 0, 0, 0)
    assert e.value.code == api.FDNN_E_STATE
    ctx.calculateUntilOutput(comp.x)
    malformed = [
        ([-1, 3], [0, 1], [4], 0),                       # seg_rows[0] < 0
        ([0, 3, 6], [1, 2, 3], [4, 5, 6], 0),            # set_ptr[0] != 0
        ([0, 10, 5], [0, 1, 2], [4, 5], 1),              # rows run backwards
        ([0, 10, 101], [0, 1, 2], [4, 5], 1),            # rows past the context
        ([0, 10, 20, 30], [0, 2, 1, 3], [4, 5, 6], 1),   # a set's range runs backwards
        ([0, 10, 20], [0, 2, 5], [1, 2, 3, 2, 7], 1),    # unsorted
        ([0, 10, 20], [0, 2, 5], [1, 2, 4, 4, 7], 1),    # a duplicate
        ([0, 10, 20], [0, 2, 4], [-1, 5, 1, 2], 0),      # negative
        ([0, 10, 20, 30], [0, 1, 2, 4], [1, 2, 5, 1000], 2),  # == O
    ]
    for seg_rows, set_ptr, nodes, seg in malformed:
        with pytest.raises(api.FdnnError) as e:
            ctx.calculateForOutputNodeSets(seg_rows, set_ptr, nodes)
        assert e.value.code == api.FDNN_E_ARG and f"segment {seg}" in str(e.value), (seg_rows, str(e.value))
    for seg_rows, set_ptr in (([-1, 3], [0, 1]), ([0, 3, 6], [1, 2, 3]), ([0, 10, 5], [0, 1, 2]), ([0, 10, 101], [0, 1, 2]),
                              ([0, 10, 20, 30], [0, 2, 1, 3])):  # the device form checks the tables (they are host memory)
        with pytest.raises(api.FdnnError) as e:
            ctx.calculateForOutputNodeSetsDevice(seg_rows, set_ptr, 0, 0, 0)
        assert e.value.code == api.FDNN_E_ARG
    ctx.delete()
    x = comp.x
    for seg_rows in ([0, 50, 99], [1, 50, 100]):  # the one-call form: seg_rows must cover [0, n)
        with pytest.raises(api.FdnnError) as e:
            dnn.calculateLazySets(x, seg_rows, [0, 1, 2], [3, 4])
        assert e.value.code == api.FDNN_E_ARG
    with pytest.raises(api.FdnnError) as e:
        dnn.calculateLazySets(x, [0, 50, 100], [0, 2, 3], [3, 3, 4])
    assert e.value.code == api.FDNN_E_ARG and "segment 0" in str(e.value)
    sr, sp, nd = np.array([0, 8], np.int32), np.array([0, 2], np.int32), np.array([1, 2], np.int32)
    p, i = np.empty(16, np.float32), np.empty(8, np.float32)
    rc = api.lib().fdnn_calculate_lazy_sets(dnn.nativeDnnHandle, x.ctypes.data_as(api._c_f32p), 8, 428, sr.ctypes.data_as(api._c_i32p),
                                            sp.ctypes.data_as(api._c_i32p), 1, nd.ctypes.data_as(api._c_i32p), p.ctypes.data_as(api._c_f32p),
                                            i.ctypes.data_as(api._c_f32p))
    assert rc == api.FDNN_E_ARG  # a wrong dim in the one-call form
