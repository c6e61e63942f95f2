"""Every return form through the model on tests/signal_nets.py's grid: small nets whose frames differ (the conditions are
tests/test_signal_nets_host.py's), at the K values that leave a wave's slice of the lazy-entry tile partly filled (240, 272,
1024, 2032 beside 16, 48, 256, 512, 2048) and behind output layers of 1, 3, 4, 31 .. 2048 nodes.

One test per (case, form).  The model and the oracle of a case are loaded once (module scope).  The references are the
oracle's taps (u8_acts, acc_out), z = softmax_ref.logits of its accumulators and float64 of those -- never the library's own
output, except where a form is DEFINED as a function of the dense rows (top-k, pooling, scores: api.*_ref of the same
call's dense rows, byte for byte) or of another entry point's bytes (set = lists, sets = set per segment, the scoring loop =
the direct call, raw frames = host-spliced rows, alignment = the restatement composed over the lazy sets call).

Every test prints its largest observed ratio to each bound ([signal-gpu] lines, run with -s); the last test prints the launch
names each case reached and asserts that the dispatch ledger knows every one of them."""
import contextlib

import numpy as np
import pytest

import align_cases as AC
import align_graph_cases as GC
import dispatch_ledger as DL
import lazy_lists_cases as LC
import lazy_set_cases as SC
import limit_nets as LN
import loglik_cases as LL
import pool_cases as PC
import signal_nets as SN
import softmax_ref as SR
from fast_dnn_amd import api, convert, formats as F
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu
CASES = SN.cases()
IDS = [SN.case_id(*c) for c in CASES]
TIGHT = 2e-6     # the project's bar, here against float64 of the oracle's logits: the reference's sequential fp32 row total is
#                  itself up to 3.5e-6 off on k1024 (O = 2048)
FUZZ = 2e-4      # tools/fuzz_parity.py's bar against the oracle's own rows
SHARES = (0.05, 0.40)
HANDLES = ((-np.inf, api.LOGLIK_F32), (-20.0, api.LOGLIK_F32), (-np.inf, api.LOGLIK_F16), (-20.0, api.LOGLIK_F16))  # tests/test_gpu_loglik.py's
ALIGN_HANDLES = ((-20.0, api.LOGLIK_F32), (-20.0, api.LOGLIK_F16))
OFFSETS = list(range(-5, 6))
ALIGNED = [c for c in CASES if SN.GRID[c[0]][0][-1] >= 3]
RAW = [c for c in CASES if c[0] in SN.RAW_DIM]

LAUNCHED = {}    # case id -> {launch name: count} over every test of the case
SET_TILE = {}    # case id -> [MFMA set launches without the walk, with it] counted by this module
FIGURES = []     # (case id, form, text)


class Ref:
    """One case: the model, the oracle, the frames and everything the oracle says about them."""

    def __init__(self, name, mode, directory):
        self.id = SN.case_id(name, mode)
        self.name, self.mode = name, mode
        path = SN.path(name, mode, directory)
        self.x = SN.features(name)
        self.orc = Oracle(path)
        self.probs, self.taps = LN.taps_mt(self.orc, self.x)
        self.hid = self.taps["u8_acts"][-1]
        self.acc = self.taps["acc_out"]
        self.z = SR.logits(self.acc, SR.coef_of(self.orc), self.orc.layer_bias(self.orc.n_layers - 1), tap=self.taps["logits"])
        self.p64 = SR.softmax64(self.z)
        self.n, self.O = self.probs.shape
        self.walk = self.orc.risky_pairs(self.orc.n_layers - 1) > 0
        assert self.walk == (mode == "gauss") and not np.isnan(self.probs).any()
        self.dnn = api.QuantizedDnn.loadFromFile(path)
        self._dense = None

    @property
    def dense(self):
        if self._dense is None:
            self._dense = self.dnn.calculate(self.x)
        return self._dense

    def masked(self, masks):
        """(z with the masked-out nodes at 0, its float64 soft-max, the oracle's lazy rows)"""
        z = np.where(masks != 0, self.z, np.float32(0.0)).astype(np.float32)
        return z, SR.softmax64(z), self.orc.output_mt(self.hid, masks=masks)


@pytest.fixture(scope="module")
def refs(tmp_models):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = Ref(case[0], case[1], tmp_models)
        return cache[case]

    yield get
    api.launch_record(False)
    for r in cache.values():
        r.dnn.delete()
        r.orc.close()


@contextlib.contextmanager
def recorded(r):
    """The launch recorder over one test of case r: its names are added to LAUNCHED[r.id]; the MFMA set kernel's counters too."""
    sb = api.set_launches()
    api.launch_record(True)
    api.launch_reset()
    try:
        yield
        got = LAUNCHED.setdefault(r.id, {})
        for k, v in api.launch_counts().items():
            got[k] = got.get(k, 0) + v
    finally:
        api.launch_record(False)
        sa = api.set_launches()
        t = SET_TILE.setdefault(r.id, [0, 0])
        t[0] += sa[0] - sb[0]
        t[1] += sa[1] - sb[1]


def note(r, form, text):
    FIGURES.append((r.id, form, text))
    print(f"\n[signal-gpu] {r.id} {form}: {text}", flush=True)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def rows_ok(r, got, z, p64, want, what):
    """The four checks of a row set: NaN pattern, softmax_ref's relative bound, 2e-6 of float64, 2e-4 of the oracle's rows
    -> (largest relative error / bound, largest |p - p64| / 2e-6, largest |p - oracle| / 2e-4)"""
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs from the oracle"
    share = SR.check(got, z, SR.rows_pad_of(r.O), what, oracle_nan=np.isnan(want))
    assert share == 0.0, f"{what}: {share:.3%} of the entries lie below 2^-126"
    rel = float((np.abs(SR.rel_err(got, p64)) / SR.bound(z, p64, SR.rows_pad_of(r.O))).max())
    e64 = float(np.abs(got.astype(np.float64) - p64).max())
    eo = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    assert e64 <= TIGHT, f"{what}: |p - float64| {e64:.3e} > {TIGHT}"
    assert eo <= FUZZ, f"{what}: |p - oracle| {eo:.3e} > {FUZZ}"
    return rel, e64 / TIGHT, eo / FUZZ


def masks_of(r, share):
    m = F.generate_masks(r.n, r.O, share, 0.03, seed=7 * r.n + int(share * 100))
    return LC._plant_special_rows(m) if r.n >= 8 else m


def device_dense(r):
    import torch

    st = torch.cuda.Stream()
    dx = torch.from_numpy(r.x).cuda()
    out = torch.full((r.n * r.O + 4,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.dnn.calculate_device(dx.data_ptr(), r.n, out.data_ptr(), st.cuda_stream)
    st.synchronize()
    got = out.cpu().numpy()
    assert (got[r.n * r.O:] == -7.0).all()
    return got[:r.n * r.O].reshape(r.n, r.O)


# ----------------------------------------------------------------------------------------------------- hidden and dense
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hidden_and_dense(refs, case):
    r = refs(case)
    with recorded(r):
        ctx = r.dnn.getNewLazyContext(r.n)
        ctx.calculateUntilOutput(r.x)
        hid = ctx.hiddenActivations()
        ctx.delete()
        assert hid.shape == r.hid.shape and np.array_equal(hid, r.hid), \
            f"{r.id}: {int((hid != r.hid).sum())} bytes of the last hidden layer differ from the oracle, first at {np.argwhere(hid != r.hid)[:1].tolist()}"
        t = r.dnn.forwardTaps(r.x)
        assert np.array_equal(t["u8_acts"], r.taps["u8_acts"]) and np.array_equal(t["acc_out"], r.acc)
        fig = rows_ok(r, r.dense, r.z, r.p64, r.probs, f"{r.id} calculate")
        dev = device_dense(r)
        fig_d = rows_ok(r, dev, r.z, r.p64, r.probs, f"{r.id} calculate_device")
    note(r, "dense", "rel/bound %.3f  |p-f64|/2e-6 %.3f  |p-oracle|/2e-4 %.4f;  device form %.3f %.3f %.4f" % (fig + fig_d))


# ----------------------------------------------------------------------------------------------------------------- masks
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_masks_as_bytes_and_bits(refs, case):
    r = refs(case)
    worst = [0.0, 0.0, 0.0]
    with recorded(r):
        for share in SHARES:
            m = masks_of(r, share)
            z, p64, want = r.masked(m)
            for form, got in (("bytes", r.dnn.calculateLazy(r.x, masks=m)), ("bits", r.dnn.calculateLazy(r.x, bits=F.pack_mask_bits(m)))):
                fig = rows_ok(r, got, z, p64, want, f"{r.id} lazy {form} {share}")
                DL._masked_out_ok(got, m, f"{r.id} lazy {form} {share}")
                worst = [max(a, b) for a, b in zip(worst, fig)]
    note(r, "masks", "rel/bound %.3f  |p-f64|/2e-6 %.3f  |p-oracle|/2e-4 %.4f" % tuple(worst))


# ----------------------------------------------------------------------------------------------------------------- lists
def lists_bound_ratio(r, m, z, p64, row_ptr, nodes, probs, inactive):
    """Largest |got / p64 - 1| / lazy_lists_cases.relative_bound over the listed entries and the inactive values."""
    got = F.lists_to_rows(row_ptr, nodes, probs, inactive, r.O)
    assert not np.isnan(got).any() and (p64 >= SR.TINY).all()
    worst = 0.0
    for f in range(r.n):
        b = LC.relative_bound(z[f], m[f] != 0, p64[f])
        rel = np.abs(got[f].astype(np.float64) / p64[f] - 1.0)
        assert (rel <= b).all(), f"{r.id} row {f}: worst rel / bound {float((rel / b).max()):.3f}"
        worst = max(worst, float((rel / b).max()))
    return worst


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lists_and_union_lists(refs, case):
    r = refs(case)
    worst, union_moved = 0.0, [0, 0, 0, 0]
    with recorded(r):
        ctx = r.dnn.getNewLazyContext(r.n)
        ctx.calculateUntilOutput(r.x)
        try:
            for share in SHARES:
                m = masks_of(r, share)
                z, p64, _ = r.masked(m)
                row_ptr, nodes = F.masks_to_lists(m)
                rows = np.repeat(np.arange(r.n), np.diff(row_ptr))
                lb = api.lists_launches()
                acc = ctx.listsAccumulators(row_ptr, nodes)
                assert np.array_equal(acc, r.acc[rows, nodes]), f"{r.id}: {int((acc != r.acc[rows, nodes]).sum())} list accumulators differ from the oracle"
                probs, inactive = ctx.calculateForOutputNodesLists(row_ptr, nodes)
                la = api.lists_launches()
                if nodes.size:  # the dot-product kernel ran, with the pair walk exactly where the layer has pairs
                    assert (la[1] > lb[1]) == r.walk and (la[0] > lb[0]) == (not r.walk) and la[2] > lb[2]
                worst = max(worst, lists_bound_ratio(r, m, z, p64, row_ptr, nodes, probs, inactive))
                op, oi = r.dnn.calculateLazyLists(r.x, row_ptr, nodes)
                assert same_bytes(op, probs) and same_bytes(oi, inactive)
                for g in (1, 2):  # the same entries on the MFMA tile over per-group unions: the dot-product lists' bytes
                    r.dnn.setListsUnion(g)
                    try:
                        ub = api.lists_union_launches()
                        up, ui = ctx.calculateForOutputNodesLists(row_ptr, nodes)
                        ua = api.lists_union_launches()
                        uacc = ctx.listsAccumulators(row_ptr, nodes)
                    finally:
                        r.dnn.setListsUnion(0)
                    assert same_bytes(up, probs) and same_bytes(ui, inactive), f"{r.id} union lists g {g} share {share}"
                    assert np.array_equal(uacc, acc)
                    moved = [a - b for a, b in zip(ua, ub)]
                    if nodes.size:  # the union's tile served it (K <= 2048), walk or walk-free as the layer says; no fallback
                        assert moved[3] == 0 and (moved[2] > 0) == r.walk and (moved[1] > 0) == (not r.walk), (r.id, g, moved)
                    union_moved = [a + b for a, b in zip(union_moved, moved)]
        finally:
            ctx.delete()
    note(r, "lists", f"rel/bound {worst:.3f}; union launches (build, walk-free, walk, fallback) {union_moved}")


# ------------------------------------------------------------------------------------------------------------------- set
def set_lengths(O):
    return sorted({1, min(O, 63), min(O, 64), min(O, 65), O})


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_set(refs, case):
    r = refs(case)
    K = SN.GRID[r.name][0][1]
    assert K <= 2048
    ranges = [(0, r.n), (7, r.n - 7)]
    with recorded(r):
        ctx = r.dnn.getNewLazyContext(r.n)
        ctx.calculateUntilOutput(r.x)
        try:
            for L in set_lengths(r.O):
                nodes = SC.pick(r.O, L, 10 + L, (0, r.O - 1))
                assert nodes[0] == 0 and (L == 1 or nodes[-1] == r.O - 1)
                for first, count in ranges:
                    rows = slice(first, first + count)
                    sb = api.set_launches()
                    probs, inactive = ctx.calculateForOutputNodeSet(nodes, first, count)
                    sa = api.set_launches()
                    # the MFMA kernel served the call, walk or walk-free as the layer says; never the list kernels
                    assert (sa[1] > sb[1]) == r.walk and (sa[0] > sb[0]) == (not r.walk) and sa[2] == sb[2], (r.id, L, first, sb, sa)
                    acc = ctx.setAccumulators(nodes, first, count)
                    assert np.array_equal(acc, r.acc[rows][:, nodes]), \
                        f"{r.id} len {L} rows {first}+{count}: {int((acc != r.acc[rows][:, nodes]).sum())} set accumulators differ from the oracle"
                    lp, li = ctx.calculateForOutputNodesLists(SC.uniform_row_ptr(count, L), np.tile(nodes, count), first=first)
                    assert same_bytes(lp.reshape(count, L), probs) and same_bytes(li, inactive), f"{r.id} len {L} rows {first}+{count}: not the list call's bytes"
        finally:
            ctx.delete()
    note(r, "set", f"K {K}: lengths {set_lengths(r.O)} x rows {ranges}: accumulators the oracle's, bytes the list call's, MFMA {'walk' if r.walk else 'walk-free'}")


# ------------------------------------------------------------------------------------------------------------------ sets
def three_segments(n):
    """Three unequal segments whose cuts lie inside 32-frame tiles."""
    cuts = [n // 5 + 1, 3 * n // 5 + 2]
    cuts = [c + 5 if c % 32 == 0 else c for c in cuts]
    seg = np.array([0, cuts[0], cuts[1], n], np.int32)
    assert (np.diff(seg) > 0).all() and len(set(np.diff(seg).tolist())) == 3 and all(c % 32 for c in cuts)
    return seg


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sets(refs, case):
    r = refs(case)
    seg = three_segments(r.n)
    sets = [SC.pick(r.O, min(r.O, L), 40 + s, (0, r.O - 1)) for s, L in enumerate((5, 70, 33))]
    set_ptr = np.concatenate([[0], np.cumsum([s.size for s in sets])]).astype(np.int32)
    with recorded(r):
        ctx = r.dnn.getNewLazyContext(r.n)
        ctx.calculateUntilOutput(r.x)
        try:
            sb = api.set_launches(), api.sets_launches()
            probs, inactive = ctx.calculateForOutputNodeSets(seg, set_ptr, np.concatenate(sets))
            sa = api.set_launches(), api.sets_launches()
            moved = [a - b for a, b in zip(sa[1], sb[1])]  # the segmented MFMA kernel served it, walk or walk-free as the layer says
            assert (moved[1] > 0) == r.walk and (moved[0] > 0) == (not r.walk) and moved[2] == 0, (r.id, moved)
            acc = ctx.setsAccumulators(seg, set_ptr, np.concatenate(sets))
            at = 0
            for s, nodes in enumerate(sets):
                a, b = int(seg[s]), int(seg[s + 1])
                p1, i1 = ctx.calculateForOutputNodeSet(nodes, a, b - a)
                blk = slice(at, at + (b - a) * nodes.size)
                assert same_bytes(probs[blk].reshape(b - a, nodes.size), p1) and same_bytes(inactive[a:b], i1), f"{r.id} segment {s}: not the set call's bytes"
                assert np.array_equal(acc[blk].reshape(b - a, nodes.size), r.acc[a:b][:, nodes]), f"{r.id} segment {s}: accumulators differ from the oracle"
                at = blk.stop
            assert at == probs.size
        finally:
            ctx.delete()
        op, oi = r.dnn.calculateLazySets(r.x, seg, set_ptr, np.concatenate(sets))
        assert same_bytes(op, probs) and same_bytes(oi, inactive)
    note(r, "sets", f"segments {seg.tolist()} lens {[s.size for s in sets]}; sets launches (walk-free, walk, by the list kernels) {moved}")


# ----------------------------------------------------------------------------------------------------------------- top-k
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_topk(refs, case):
    r = refs(case)
    kept = {}
    with recorded(r):
        dense = r.dense
        for k in sorted({1, min(5, r.O), min(r.O, 256)}):
            nodes, probs = r.dnn.calculateTopK(r.x, k)
            wn, wp = api.topk_ref(dense, k)
            assert same_bytes(nodes, wn) and same_bytes(probs, wp), f"{r.id} top-{k}: not the selection of the same call's dense rows"
            rows = SN.topk_rows(r.probs, k)  # where the oracle's k-th and (k+1)-th are apart, the node SET is the oracle's
            want = np.sort(np.argsort(-r.probs.astype(np.float64), axis=1, kind="stable")[:, :k], axis=1)
            got = np.sort(nodes, axis=1)
            assert np.array_equal(got[rows], want[rows]), f"{r.id} top-{k}: {int((got[rows] != want[rows]).any(1).sum())} rows differ from the oracle's top-{k} set"
            kept[k] = float(rows.mean())
    note(r, "topk", "rows held to the oracle's set per k: " + ", ".join(f"{k}: {v:.1%}" for k, v in kept.items()))


# ------------------------------------------------------------------------------------------------------------------ pool
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pool(refs, case):
    r = refs(case)
    worst = 0.0
    p = r.probs.astype(np.float64)
    with recorded(r):
        dense = r.dense
        for mk in ("interleaved", "one"):
            co, C = PC.map_of(mk, r.O, classes=min(r.O, 7))
            assert C == (1 if mk == "one" else min(r.O, 7))
            pool = api.ClassPool(co, C)
            try:
                q = r.dnn.calculatePool(r.x, pool)
            finally:
                pool.delete()
            assert PC.same_bytes(q, api.pool_ref(dense, co, C)), f"{r.id} {mk}: not the pool of the same call's dense rows"
            for c, m in enumerate(PC.members(co, C)):
                exact = p[:, m].sum(1)
                bound = PC.oracle_bound(m.size, exact, LC.TIGHT)
                err = np.abs(q[:, c].astype(np.float64) - exact)
                assert (err <= bound).all(), (r.id, mk, c, m.size, float(err.max()), float(bound.min()))
                worst = max(worst, float((err / bound).max()))
    note(r, "pool", f"largest |q - oracle sum| / bound {worst:.4f}")


# ---------------------------------------------------------------------------------------------------------------- scores
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_scores(refs, case):
    r = refs(case)
    lp = LL.priors(r.O)
    got = {}
    with recorded(r):
        dense = r.dense
        for floor, t in HANDLES:
            ll = api.Loglik(lp, floor, t)
            try:
                got[(floor, t)] = r.dnn.calculateLoglik(r.x, ll)
            finally:
                ll.delete()
            want = api.loglik_ref(dense, lp, floor, t)
            assert got[(floor, t)].dtype == want.dtype and LL.same_bytes(got[(floor, t)], want), f"{r.id} {floor} {t}: not the scores of the same call's dense rows"
    ratio = LL.assert_log_of_rows(dense, lp, got[(-np.inf, api.LOGLIK_F32)], got[(-np.inf, api.LOGLIK_F16)])
    note(r, "scores", f"|s - (ln dense - prior)| / bound {ratio:.3f}")


# ------------------------------------------------------------------------------------------------------------- alignment
@pytest.mark.parametrize("case", ALIGNED, ids=[SN.case_id(*c) for c in ALIGNED])
def test_align(refs, case):
    r = refs(case)
    seg_rows = AC.seg_rows_of(r.n, 2)
    ptr, states = AC.transcripts(r.probs, seg_rows, 31)  # from the runs of the ORACLE rows' arg-max
    assert (np.diff(ptr) < np.diff(seg_rows)).all() and np.unique(states).size < states.size
    sl, nl = AC.transitions(states.size, 32)
    lp = LL.priors(r.O)
    fracs = []
    with recorded(r):
        ctx = r.dnn.getNewLazyContext(r.n)
        ctx.calculateUntilOutput(r.x)
        try:
            for handle in ALIGN_HANDLES:
                ll = api.Loglik(lp, *handle)
                try:
                    want = AC.composed(r.dnn, r.x, lp, handle, seg_rows, ptr, states, sl, nl)
                    assert np.isfinite(want[1]).all()
                    for s in range(seg_rows.size - 1):  # the comparison is not blind: the path is far from the uniform segmentation
                        p = want[0][seg_rows[s]:seg_rows[s + 1]]
                        frac = AC.differ(p, AC.uniform_path(p.size, int(ptr[s + 1] - ptr[s])))
                        fracs.append(frac)
                        assert frac >= 0.25, (r.id, s, frac)
                    assert AC.same(r.dnn.calculateAlign(r.x, ll, seg_rows, ptr, states, sl, nl), want), (r.id, handle)
                    assert AC.same(ctx.align(ll, seg_rows, ptr, states, sl, nl), want), (r.id, handle)
                finally:
                    ll.delete()
        finally:
            ctx.delete()
    note(r, "align", f"arg-max runs {SN.arg_max_runs(r.probs)}, T {np.diff(seg_rows).tolist()} S {np.diff(ptr).tolist()}, off the uniform segmentation {min(fracs):.0%} .. {max(fracs):.0%}")


@pytest.mark.parametrize("case", ALIGNED, ids=[SN.case_id(*c) for c in ALIGNED])
def test_align_graph(refs, case):
    r = refs(case)
    seg_rows = AC.seg_rows_of(r.n, 2)
    graphs = GC.silence_graphs(r.probs, seg_rows, 31)  # optional-silence graphs over the runs of the ORACLE rows' arg-max
    packed = api.pack_graphs(graphs)
    lp = LL.priors(r.O)
    with recorded(r):
        ctx = r.dnn.getNewLazyContext(r.n)
        ctx.calculateUntilOutput(r.x)
        try:
            for handle in ALIGN_HANDLES:
                ll = api.Loglik(lp, *handle)
                try:
                    want, pieces = GC.composed(r.dnn, r.x, lp, handle, seg_rows, packed)
                    assert np.isfinite(want[1]).all()
                    GC.not_blind(r.id, want, pieces, seg_rows, graphs)
                    assert AC.same(r.dnn.calculateAlignGraph(r.x, ll, seg_rows, packed), want), (r.id, handle)
                    assert AC.same(ctx.alignGraph(ll, seg_rows, packed), want), (r.id, handle)
                finally:
                    ll.delete()
        finally:
            ctx.delete()
    note(r, "align_graph", f"T {np.diff(seg_rows).tolist()} S {[len(g['states']) for g in graphs]}: both entry points return the restatement's path and total")


# ------------------------------------------------------------------------------------------------------------ raw frames
@pytest.mark.parametrize("case", RAW, ids=[SN.case_id(*c) for c in RAW])
def test_raw_frames(refs, case):
    r = refs(case)
    raw_dim, D = SN.RAW_DIM[r.name], r.x.shape[1]
    raw = (np.random.default_rng(87).standard_normal((r.n, raw_dim)) * 19.9 + 1.9).astype(np.float32)  # synth_features' statistics
    rows = convert.splice_frames(raw, OFFSETS, D)
    assert rows.shape == (r.n, D) and len(np.unique(r.orc.hidden_acts_mt(rows), axis=0)) == r.n  # these frames differ too
    lp = LL.priors(r.O)
    with recorded(r):
        r.dnn.setSplice(OFFSETS, raw_dim)
        try:
            dense = r.dnn.calculate(rows)
            assert same_bytes(r.dnn.calculateRaw(raw), dense), f"{r.id}: calculateRaw differs from calculate on the host-spliced rows"
            for floor, t in ((-20.0, api.LOGLIK_F16), (-np.inf, api.LOGLIK_F32)):
                ll = api.Loglik(lp, floor, t)
                try:
                    assert LL.same_bytes(r.dnn.calculateLoglikRaw(raw, ll), r.dnn.calculateLoglik(rows, ll)), (r.id, floor, t)
                finally:
                    ll.delete()
        finally:
            r.dnn.setSplice([], 0)
    want = r.orc.output_mt(r.orc.hidden_acts_mt(rows))
    assert float(np.abs(dense - want).max()) <= FUZZ  # and the spliced rows' result is the oracle's
    note(r, "raw", f"raw width {raw_dim} x 11 -> {D}: calculateRaw and calculateLoglikRaw return the host-spliced rows' bytes")


# ---------------------------------------------------------------------------------------------------------- scoring loop
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_scoring_loop(refs, case):
    r = refs(case)
    nodes = SC.pick(r.O, min(r.O, 65), 75, (0, r.O - 1))
    with recorded(r):
        dense = r.dense
        sp, si = r.dnn.calculateLazySet(r.x, nodes)
        srv = api.ScoringServer(r.dnn, max(r.n, 64), 2)
        try:
            t, out = srv.submit(r.x)
            srv.wait(t)
            assert same_bytes(out, dense), f"{r.id}: the loop's dense rows differ from calculate's"
            t, p, i = srv.submitLazySet(r.x, nodes)
            srv.wait(t)
            assert same_bytes(p, sp) and same_bytes(i, si), f"{r.id}: the loop's set rows differ from calculateLazySet's"
        finally:
            srv.close()
    assert same_bytes(r.dnn.calculate(r.x), dense)  # the dense entry point keeps its bytes
    note(r, "loop", "a dense and a lazy-set submission: the direct calls' bytes")


# ---------------------------------------------------------------------------------------------------- launch-name report
def test_every_launch_name_the_grid_reaches_is_in_the_ledger(refs):
    """Runs last in this file: per case the launch names its tests reached, and the MFMA set tile's counters.  A name the
    ledger's cases never launch is a finding: a kernel instance only this grid reaches."""
    assert LAUNCHED, "no test of this module has run before this one"
    known = set().union(*DL.EXPECT.values())
    table = set(api.launch_names())
    reached = set()
    for cid in sorted(LAUNCHED):
        names = LAUNCHED[cid]
        reached |= set(names)
        print(f"\n[signal-gpu] {cid} launch names: {' '.join(sorted(names))}", flush=True)
        print(f"[signal-gpu] {cid} MFMA set tile launches: walk-free {SET_TILE.get(cid, [0, 0])[0]}, walk {SET_TILE.get(cid, [0, 0])[1]}", flush=True)
    assert reached <= table
    unknown = sorted(reached - known)
    assert not unknown, f"launch names no ledger case covers: {unknown}"
    # the set / sets tile ran at every K of the grid, in the walk form on gauss and the walk-free form on nosat
    if len(SET_TILE) == len(CASES):
        for name, mode in CASES:
            free, walk = SET_TILE[SN.case_id(name, mode)]
            assert (walk > 0 and free == 0) if mode == "gauss" else (free > 0 and walk == 0), (name, mode, free, walk)
