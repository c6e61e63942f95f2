"""One context, many calls.  Every other GPU test makes a context, calls it once and deletes it; a
production caller's pooled contexts and scoring-loop slots live for the whole process and serve a different batch every time.
What a launch leaves behind for the NEXT one -- the self-rewinding counters scr_count, fuse_cnt, fuse_flag, chain_ctl and
chain_done, the rows of a larger batch past a smaller one's last frame, the host-side notes of the call before -- is what
this file is about.  The rule of every step of every sequence:

  * the kernel families the step will launch are PREDICTED from the selection rules themselves (tests/host/select_query.cpp,
    built here from fdnn_select.hpp) and the prediction is held against the launch recorder, in both directions;
  * what it computes is the oracle's: last hidden bytes bit for bit, soft-max rows through the ledger's _softmax_ok /
    _softmax_rel_ok (lists, sets and top-k rebuilt into rows first), masked-out entries one value per row;
  * the scratch audit of the context is clean and the model's fault counters stand where they stood BEFORE the next step is
    launched -- no launch is ever made onto counters known to be dirty --, and a failure names the step and its predecessor.

The sizes, as verified with the selection query (an explicit context has a fixed frame count, so the sequences that change n
on ONE explicit context run on a SpliceStream's: its context takes every utterance's length; rows are the spliced raw frames):

  a  fuse_cnt across its two layouts, net full/gauss, fuse forced: role-split (ppo.out) at n = 641 -- three 320-frame pairs,
     the last with one frame and an all-padding half --, in-phase (gemm.out.ft128.bk128, 8 words per 128-frame tile) on the
     same 641 frames, role-split at 1281, in-phase at 1025 -- the smallest n at which frame_tile's cost model answers another
     tile (256) --, role-split at 641 again.
  b  scr_count across its geometries, net mid, ONE explicit context of 2048 frames (the screened kernel needs n >= 2048:
     choose_l0's can_screen), flagged-output list capped at 3000: int8 screening with every fifth row NaN (whole-tile path by
     list overflow); with 77 of one 128-frame tile's rows NaN (60 %: at this size the screening runs 64-node tiles, 128 x 64
     outputs, so 40 % of the rows stay below kL0ScreenCap = 4096 and 60 % exceed it); the screened kernel on the same two
     batches (its per-tile lists, and the whole tile where 77 x 128 > 4096); both on clean rows.  The screened kernel's
     64-frame tiles exist in measurement builds only (l0.screen.f64 carries the ablation flag: asserted below), so that
     geometry has no step.
  c  chain_done across strides and tiles, chain forced: 256-wide net with two int8 hidden layers at n = 500 (256-frame
     tiles), 600 (320), 130 (one tile), 1500; limit_nets' 9-layer net (a pass = an 8-layer and a 1-layer launch on the same
     words) at 600 twice, then 500.
  d  one POOLED context shrinking and growing, net full/gauss: n = 513 (the ledger's smallest fused shape), 1, 512, 65, 64,
     321, 513, 65 through calculate, calculateLazy (bytes, then bits), the list call, the list call over unions, the set
     call, calculateTopK, calculateRaw.
  e  every output kind behind one hidden pass, net mid: 300 frames, then 100 with the kinds in reverse.
  f  a seeded walk: 24 steps on the 256-wide net, 8 on the full net.
  g  the scoring loop's slots.

Which step catches a kernel that skipped a buffer's rewind: scr_count -- b1 (int8 screening, whole-tile path) and b3 / b4
(screened kernel); fuse_cnt -- a1 (role-split layout) and a2 (in-phase layout); fuse_flag -- only a give-up raises one, and
the one give-up run is test_gpu_production_shapes.py's child, which prints this audit; chain_ctl and chain_done -- c1."""
import os
import subprocess

import numpy as np
import pytest

import dispatch_ledger as DL
import lazy_set_cases as LS
import limit_nets as LN
from conftest import ROOT
from dispatch_ledger import TIGHT, _masked_out_ok, _softmax_ok, _softmax_rel_ok, launched
from fast_dnn_amd import api, convert as CV, formats as F
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

KALDI = (list(range(-5, 6)), 39)
NAMES = ("scr_count", "fuse_cnt", "fuse_flag", "chain_ctl", "chain_done")
FAMILIES = ("l0.", "chain.", "gemm.hid.", "small.hid.", "pp.hid.", "gemm.out.", "small.out.", "ppo.out.")
# net -> (ledger kind or None, D, H, int8 hidden layers, O, has saturating pairs)
SHAPES = {"n256": ("n256/256/gauss", 432, 256, 2, 256, 1), "mid": ("mid", 432, 256, 2, 1000, 1), "full": ("full/gauss", 432, 2048, 6, 8000, 1),
          "deep9": (None, 432, 256, 9, 252, 1)}


# ------------------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(scope="module")
def query(tmp_path_factory):
    """query(net, n, kind, fuse, chain, ppo, l0k) -> ({"l0": [...], "hid": [...], "out": [...]}, fused or None): the
    launch-name prefixes the selection rules choose (tests/host/select_query.cpp)."""
    exe = str(tmp_path_factory.mktemp("select_query") / "select_query")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "fast-dnn_amd", "csrc"), os.path.join(ROOT, "tests", "host", "select_query.cpp"),
                         "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    cache = {}

    def ask(net, n, kind, fuse, chain, ppo, l0k):
        key = (net, n, kind, fuse, chain, ppo, l0k)
        if key not in cache:
            _, D, H, n_hid, O, fix = SHAPES[net]
            run = subprocess.run([exe, f"{D},{H},{n_hid},{O},{fix},{n},{fuse},{chain},{ppo},{l0k},{kind}"], capture_output=True, text=True)
            assert run.returncode == 0, run.stderr
            parts, fused = {"l0": [], "hid": [], "out": []}, None
            for tok in run.stdout.split():
                if tok in ("fused", "unfused"):
                    fused = tok == "fused"
                else:
                    parts["l0" if tok.startswith("l0.") else "out" if ".out." in tok else "hid"].append(tok)
            cache[key] = (parts, fused)
        return cache[key]

    return ask


class Net:
    """A model, its oracle and -- per frame count -- the spliced rows of one seeded raw utterance with the oracle's answers."""

    def __init__(self, name, path):
        self.name, self.path = name, path
        self.dnn = api.QuantizedDnn.loadFromFile(path, device=0)
        self.orc = Oracle(path)
        self.dnn.setSplice(*KALDI)
        self.O, self.H = self.dnn.outputDimension(), self.dnn.hiddenDimension()
        self.raw = np.ascontiguousarray(F.synth_features(2048, 432, seed=2000 + len(name))[:, :KALDI[1]])
        self._ref = {}

    def rows_of(self, n):
        """Rows the oracle scores: all of them on the 256-wide nets; on the 2048-wide net row 0, row n - 1, both sides of the
        tile edges (128, 160, 256, 320 and their multiples nearest n / 2 and n) and 16 seeded rows."""
        if self.H <= 256:
            return np.arange(n)
        pick = {0, n - 1}
        for tile in (128, 160, 256, 320):
            for target in (tile, n / 2, n):
                m = int(round(target / tile)) * tile
                pick |= {r for r in (m - 1, m) if 0 <= r < n}
        rng = np.random.default_rng(n)
        pick |= {int(r) for r in rng.integers(0, n, 16)}
        return np.array(sorted(pick))

    def ref(self, n, x=None, tag=""):
        """-> dict(x [n][432], idx, hid, want, acc) for the n-frame utterance raw[:n] (or the rows x under a tag of their own)."""
        key = (n, tag)
        if key not in self._ref:
            if x is None:
                x = CV.splice_frames(self.raw[:n], KALDI[0], 432)
            idx = self.rows_of(n)
            with np.errstate(all="ignore"):
                hid = self.orc.hidden_acts_mt(x[idx])
                want, acc = self.orc.output_mt(hid, want_acc=True)
            self._ref[key] = dict(x=np.ascontiguousarray(x), idx=idx, hid=hid, want=want, acc=acc)
        return self._ref[key]

    def counters(self):
        return self.dnn.chainFaults(), int(self.dnn.deviceCounters(4)[3]), self.dnn.fuseGiveups()

    def close(self):
        self.dnn.setSplice([], 0)
        self.dnn.delete()
        self.orc.close()


@pytest.fixture(scope="module")
def nets(tmp_models, mid_model_path, net_model_path):
    cache = {}

    def get(name):
        if name not in cache:
            if name == "mid":
                path = mid_model_path
            elif name == "full":
                path = net_model_path
            elif name == "deep9":
                path = LN.cached(tmp_models, "seq_deep9", LN.deep_topology(9), lambda: LN.deep_net(9))
            else:
                path = DL.net_path(SHAPES[name][0])
            cache[name] = Net(name, path)
        return cache[name]

    yield get
    for net in cache.values():
        net.close()


@pytest.fixture(autouse=True)
def modes():
    yield
    api.scratch_audit(False)
    api.scratch_dirty()
    api.launch_record(False)
    api.set_fuse(-1)
    api.set_chain(-1)
    api.set_pp(-1)
    api.set_ppo(-1)


class Walk:
    """The steps of one sequence on one model.  audit: () -> {buffer: non-zero words} of the context(s) the step used."""

    def __init__(self, net, query, audit):
        self.net, self.query, self.audit = net, query, audit
        self.prev = "(a fresh context)"
        self.trace = []

    def step(self, label, run, n, kind, parts, fuse=1, chain=0, ppo=-1, l0k=0):
        """run() under the recorder with the modes set; predicted families == launched families; audit clean; counters
        unchanged -> run's result."""
        what = f"step '{label}' (after {self.prev})"
        self.trace.append(label)
        api.set_fuse(fuse)
        api.set_chain(chain, 1 if chain else 0)
        api.set_ppo(ppo)
        self.net.dnn.setInputLayerKernel(l0k)
        before = self.net.counters()
        try:
            res, ran = launched(run)
        finally:
            self.net.dnn.setInputLayerKernel(0)
        # ---- the counters first: nothing else is launched on this context unless they are where they were
        state = self.audit()
        dirty = {k: v for k, v in state.items() if k in NAMES and v}
        assert not dirty, f"{what}: scratch audit: counters left non-zero (buffer: words) {dirty}; sequence so far: {self.trace}"
        after = self.net.counters()
        assert after[:2] == before[:2], f"{what}: a chained launch ran into its wait bound: (chainFaults, device counter [3]) {before[:2]} -> {after[:2]}"
        assert after[2] == before[2], f"{what}: fused soft-max tiles gave up waiting: fuseGiveups {before[2]} -> {after[2]}"
        # ---- the instance: predicted by the selection rules, asserted with the recorder
        pred, fused = self.query(self.net.name, n, kind, fuse, chain, ppo, l0k)
        want = [p for part in parts for p in pred[part]]
        fam = {k for k in ran if k.startswith(FAMILIES)}
        for p in want:
            assert any(k.startswith(p) for k in fam), f"{what}: the selection predicts {p}*, launched: {sorted(ran)}"
        for k in fam:
            assert any(k.startswith(p) for p in want), f"{what}: launched {k}, which the selection does not predict ({want})"
        if "out" in parts and fused is not None:
            for k in fam:
                if k.startswith("gemm.out."):
                    assert ("fused" in k) == fused, f"{what}: predicted {'fused' if fused else 'unfused'}, launched {k}"
        self.prev = f"'{label}'"
        return res


def ctx_audit(ctx_of):
    return lambda: ctx_of().scratchState()


def pool_audit(contexts=1):
    """Totals of the process-wide audit since the last look: the pooled context the step drew and gave back."""
    def look():
        t = api.scratch_dirty()
        assert t["unreadable"] == 0 and t["contexts"] >= contexts, f"the audit looked at {t['contexts']} contexts (at least {contexts} expected)"
        return t
    return look


def masks_for(n, O, seed):
    m = F.generate_masks(n, O, 0.40, 0.03, seed=seed)
    if n >= 8:
        m[1] = 1  # a full row
        m[2] = 0  # an empty one
    return m


def check_hidden(net, r, got, what):
    assert np.array_equal(got[r["idx"]], r["hid"]), f"{what}: last hidden layer's bytes differ from the oracle"


def check_dense(net, r, got, what):
    _softmax_ok(got[r["idx"]], r["want"], what + " dense")
    _softmax_rel_ok(got[r["idx"]], r["want"], net.orc, r["acc"], what + " dense")


def check_lazy(net, r, got, masks, what):
    m = masks[r["idx"]]
    with np.errstate(all="ignore"):
        want = net.orc.output_mt(r["hid"], masks=m)
    _softmax_ok(got[r["idx"]], want, what)
    _softmax_rel_ok(got[r["idx"]], want, net.orc, r["acc"], what, masks=m)
    _masked_out_ok(got[r["idx"]], m, what)


def rows_of_lists(rp, nd, probs, inactive, masks, O):
    """A list call's rows; a row that lists every node has no reader for its inactive value."""
    full = np.diff(rp) == O
    inactive = np.where(full, np.float32(1.0), inactive)
    return F.lists_to_rows(rp, nd, probs, inactive, O)


def rows_of_set(nodes, probs, inactive, O):
    out = np.repeat(np.asarray(inactive, np.float32)[:, None], O, axis=1)
    out[:, nodes] = probs
    return out


def set_masks(n, O, nodes):
    m = np.zeros((n, O), np.int8)
    m[:, nodes] = 1
    return m


def check_topk(net, r, nodes, probs, k, what):
    """Against the oracle (tests/test_gpu_topk.py's bar): every returned value is a 2e-6 probability of its node, values do
    not ascend, and no node left out beats the smallest one returned by more than 4e-6."""
    idx, want = r["idx"], r["want"]
    nd, pr = nodes[idx], probs[idx]
    assert nd.shape == (idx.size, k) and (nd >= 0).all() and (nd < net.O).all(), what
    assert all(np.unique(row).size == k for row in nd), f"{what}: a node returned twice"
    assert np.abs(pr - np.take_along_axis(want, nd.astype(np.int64), axis=1)).max() <= TIGHT, f"{what}: a returned value is not its node's probability"
    assert (np.diff(pr, axis=1) <= 0).all(), f"{what}: values ascend"
    rest = want.copy()
    np.put_along_axis(rest, nd.astype(np.int64), -np.inf, axis=1)
    assert (rest.max(1) <= pr[:, -1] + 2 * TIGHT).all(), f"{what}: a node left out beats the smallest one returned"


class Streamed:
    """The explicit context of a SpliceStream: one context whose frame count is every utterance's."""

    def __init__(self, net, max_chunk):
        self.net = net
        self.st = net.dnn.newStream(max_chunk)
        self.ctx = None

    def hidden(self, n):
        self.st.reset()
        self.ctx = self.st.pushHidden(self.net.raw[:n], end=True)
        assert self.ctx.inputVectorCount == n
        return self.ctx

    def view(self):
        return self.ctx if self.ctx is not None else api.LazyContext(self.net.dnn, api.lib().fdnn_stream_ctx(self.st.handle), 0, owned=False)

    def close(self):
        self.st.close()


# ------------------------------------------------------------------------------------------- a. fuse_cnt, two layouts
def test_a_fuse_counters_across_the_role_split_and_the_in_phase_layout(nets, query):
    net = nets("full")
    s = Streamed(net, 1281)
    w = Walk(net, query, ctx_audit(s.view))
    try:
        for i, (n, ppo, rehid) in enumerate(((641, 1, True), (641, 0, False), (1281, 1, True), (1025, 0, True), (641, 1, True)), 1):
            r = net.ref(n)
            form = "role-split" if ppo else "in-phase"
            if rehid:
                ctx = w.step(f"a{i} hidden layers, n = {n}", lambda: s.hidden(n), n, "none", ("l0", "hid"))
                check_hidden(net, r, ctx.hiddenActivations(), f"a{i} n = {n}")
            pred, fused = query("full", n, "dense", 1, 0, ppo, 0)
            assert fused and pred["out"] == (["ppo.out."] if ppo else ["gemm.out.ft256." if n == 1025 else "gemm.out.ft128.bk128."]), (n, ppo, pred)
            got = w.step(f"a{i} dense output, {form}, n = {n}", lambda: s.ctx.calculateOutput(), n, "dense", ("out",), ppo=ppo)
            check_dense(net, r, got, f"a{i} {form} n = {n}")
    finally:
        s.close()


# --------------------------------------------------------------------------------------------- b. scr_count, geometries
def test_b_screening_counters_across_the_kernels_that_share_them(nets, query):
    assert api.launch_names()["l0.screen.f64"] & api.LAUNCH_ABLATION, "the screened kernel's 64-frame tiles are launchable: give them a step"
    net = nets("mid")
    n, cap = 2048, 3000
    base = net.ref(n)["x"]
    nan5 = base.copy()
    nan5[::5] = np.float32("nan")
    nan_tile = base.copy()
    nan_tile[384 + np.random.default_rng(5).choice(128, 77, replace=False)] = np.float32("nan")  # 60 % of frame tile 3
    batches = {"every fifth row NaN": ("nan5", nan5), "77 rows of one tile NaN": ("nantile", nan_tile), "clean rows": ("", base)}
    net.dnn.setInputLayerListCap(cap)
    ctx = fresh = None
    try:
        ctx = net.dnn.getNewLazyContext(n)
        w = Walk(net, query, ctx_audit(lambda: ctx))
        recomputed = {}
        steps = ((4, "every fifth row NaN"), (4, "77 rows of one tile NaN"), (3, "every fifth row NaN"), (3, "77 rows of one tile NaN"), (3, "clean rows"),
                 (4, "clean rows"))
        for i, (l0k, which) in enumerate(steps, 1):
            tag, x = batches[which]
            r = net.ref(n, x=x, tag=tag) if tag else net.ref(n)
            label = f"b{i} {'int8 screening' if l0k == 4 else 'screened kernel'}, {which}"
            pred, _ = query("mid", n, "none", 1, 0, -1, l0k)
            assert pred["l0"] == (["l0.digits", "l0.split.n64", "l0.fixlist.lpo8"] if l0k == 4 else ["l0.screen.f128", "l0.fix.tiles"]), pred
            before = int(net.dnn.deviceCounters(4)[1])
            w.step(label, lambda: ctx.calculateUntilOutput(x), n, "none", ("l0", "hid"), l0k=l0k)
            recomputed[i] = int(net.dnn.deviceCounters(4)[1]) - before
            check_hidden(net, r, ctx.hiddenActivations(), label)
        nan_outputs = int(np.isnan(nan5).any(1).sum()) * net.H
        assert recomputed[1] >= nan_outputs > cap, f"b1: {recomputed[1]} outputs recomputed, {nan_outputs} are NaN rows': the capped list ({cap}) did not overflow"
        assert recomputed[2] >= 128 * 128 and recomputed[4] >= 128 * 128, f"b2 / b4: the tile with 77 NaN rows was not recomputed whole ({recomputed[2]}, {recomputed[4]})"
        # a stale count is invisible in the bytes: it only makes the next launch recompute a tile whole.  The clean steps
        # recompute exactly what a fresh context recomputes for the same batch.
        for i, l0k in ((5, 3), (6, 4)):
            fresh = net.dnn.getNewLazyContext(n)
            net.dnn.setInputLayerKernel(l0k)
            before = int(net.dnn.deviceCounters(4)[1])
            fresh.calculateUntilOutput(base)
            first = int(net.dnn.deviceCounters(4)[1]) - before
            net.dnn.setInputLayerKernel(0)
            assert fresh.scratchState() == dict.fromkeys(NAMES, 0)
            fresh.delete()
            fresh = None
            if l0k == 4:
                assert first < cap, f"{first} flagged outputs on clean rows do not fit the capped list ({cap}): which tiles overflow is a race, the counts cannot be compared"
            assert 0 < first == recomputed[i], f"b{i}: {recomputed[i]} outputs recomputed on the used context, {first} on a fresh one"
    finally:
        net.dnn.setInputLayerKernel(0)
        for c in (ctx, fresh):
            if c is not None:
                c.delete()
        net.dnn.setInputLayerListCap(0)


# ------------------------------------------------------------------------------------------ c. chain_done, strides, tiles
@pytest.mark.parametrize("name,sizes", [("n256", (500, 600, 130, 1500)), ("deep9", (600, 600, 500))], ids=["two_layers", "nine_layers"])
def test_c_chain_counters_across_strides_and_frame_tiles(nets, query, name, sizes):
    net = nets(name)
    s = Streamed(net, max(sizes))
    w = Walk(net, query, ctx_audit(s.view))
    try:
        for i, n in enumerate(sizes, 1):
            pred, _ = query(name, n, "none", 1, 1, -1, 0)
            assert pred["hid"] == [f"chain.ft{DL.chain_tile(n)}."], pred
            label = f"c{i} chained hidden layers, n = {n} ({DL.chain_tile(n)}-frame tiles)"
            (ctx, launches) = w.step(label, lambda: (s.hidden(n), dict(api.launch_counts())), n, "none", ("l0", "hid"), chain=1)
            chained = sum(v for k, v in launches.items() if k.startswith("chain."))
            assert chained == (2 if name == "deep9" else 1), f"{label}: {chained} chained launches ({launches})"
            check_hidden(net, net.ref(n), ctx.hiddenActivations(), label)
        assert net.dnn.chainFaults() == 0
    finally:
        s.close()


# ------------------------------------------------------------------------------- d. one pooled context, shrinking, growing
def test_d_one_pooled_context_serves_every_entry_point_at_every_size(nets, query):
    net = nets("full")
    dnn, O = net.dnn, net.O
    C = 513
    api.scratch_dirty()
    api.scratch_audit(True)
    w = Walk(net, query, pool_audit())
    union_before = api.lists_union_launches()

    def entry(kind, n, r):
        x = r["x"]
        masks = masks_for(n, O, seed=40 + n)
        rp, nd = F.masks_to_lists(masks)
        nodes = LS.pick(O, 70, 60 + n, (0, O - 1))
        what = f"d {kind} n = {n}"
        if kind == "calculate":
            check_dense(net, r, w.step(what, lambda: dnn.calculate(x), n, "dense", ("l0", "hid", "out")), what)
        elif kind in ("lazy bytes", "lazy bits"):
            call = (lambda: dnn.calculateLazy(x, masks=masks)) if kind == "lazy bytes" else (lambda: dnn.calculateLazy(x, bits=F.pack_mask_bits(masks)))
            check_lazy(net, r, w.step(what, call, n, "bits", ("l0", "hid", "out")), masks, what)
        elif kind in ("lists", "lists over unions"):
            dnn.setListsUnion(1 if kind == "lists over unions" else 0)
            try:
                probs, inactive = w.step(what, lambda: dnn.calculateLazyLists(x, rp, nd), n, "none", ("l0", "hid"))
            finally:
                dnn.setListsUnion(0)
            check_lazy(net, r, rows_of_lists(rp, nd, probs, inactive, masks, O), masks, what)
        elif kind == "set":
            probs, inactive = w.step(what, lambda: dnn.calculateLazySet(x, nodes), n, "none", ("l0", "hid"))
            check_lazy(net, r, rows_of_set(nodes, probs, inactive, O), set_masks(n, O, nodes), what)
        elif kind == "top-k":
            tn, tp = w.step(what, lambda: dnn.calculateTopK(x, 32), n, "dense", ("l0", "hid", "out"))
            check_topk(net, r, tn, tp, 32, what)
        else:
            check_dense(net, r, w.step(what, lambda: dnn.calculateRaw(net.raw[:n]), n, "dense", ("l0", "hid", "out")), what)

    for n, kind in ((C, "calculate"), (1, "lazy bytes"), (C - 1, "lazy bits"), (65, "lists"), (64, "lists over unions"), (321, "set"), (C, "top-k"), (65, "raw")):
        entry(kind, n, net.ref(n))
    assert api.lists_union_launches()[0] > union_before[0], "the list call with setListsUnion(1) did not take the union path"
    pred, fused = query("full", C, "dense", 1, 0, -1, 0)
    assert fused and pred["out"] == ["gemm.out.ft128.bk128."], pred  # C is a fused shape: the pooled context's fuse counters were in use


# ------------------------------------------------------------------------------ e. every output kind behind one hidden pass
def test_e_every_output_kind_behind_one_hidden_pass(nets, query):
    net = nets("mid")
    dnn, O = net.dnn, net.O
    s = Streamed(net, 300)
    w = Walk(net, query, ctx_audit(s.view))
    kinds = ("dense", "byte masks", "bit masks", "lists", "union lists", "set", "sets", "top-k", "dense again")
    try:
        for n, order in ((300, kinds), (100, kinds[::-1])):
            r = net.ref(n)
            ctx = w.step(f"e hidden layers, n = {n}", lambda: s.hidden(n), n, "none", ("l0", "hid"))
            check_hidden(net, r, ctx.hiddenActivations(), f"e n = {n}")
            masks = masks_for(n, O, seed=70 + n)
            rp, nd = F.masks_to_lists(masks)
            a, b = LS.pick(O, 70, 71, (0, O - 1)), LS.pick(O, 129, 72, (O - 1,))
            for kind in order:
                what = f"e {kind}, n = {n}"
                if kind.startswith("dense"):
                    check_dense(net, r, w.step(what, ctx.calculateOutput, n, "dense", ("out",)), what)
                elif kind == "byte masks":
                    check_lazy(net, r, w.step(what, lambda: ctx.calculateForOutputNodesBatch(masks), n, "bytes", ("out",)), masks, what)
                elif kind == "bit masks":
                    check_lazy(net, r, w.step(what, lambda: ctx.calculateForOutputNodesBatchBits(F.pack_mask_bits(masks)), n, "bits", ("out",)), masks, what)
                elif kind in ("lists", "union lists"):
                    dnn.setListsUnion(1 if kind == "union lists" else 0)
                    try:
                        probs, inactive = w.step(what, lambda: ctx.calculateForOutputNodesLists(rp, nd), n, "none", ())
                    finally:
                        dnn.setListsUnion(0)
                    check_lazy(net, r, rows_of_lists(rp, nd, probs, inactive, masks, O), masks, what)
                elif kind == "set":
                    probs, inactive = w.step(what, lambda: ctx.calculateForOutputNodeSet(a), n, "none", ())
                    check_lazy(net, r, rows_of_set(a, probs, inactive, O), set_masks(n, O, a), what)
                elif kind == "sets":
                    cut = 33
                    probs, inactive = w.step(what, lambda: ctx.calculateForOutputNodeSets([0, cut, n], [0, a.size, a.size + b.size], np.concatenate((a, b))), n, "none", ())
                    rows = np.concatenate((rows_of_set(a, probs[:cut * a.size].reshape(cut, a.size), inactive[:cut], O),
                                           rows_of_set(b, probs[cut * a.size:].reshape(n - cut, b.size), inactive[cut:], O)))
                    check_lazy(net, r, rows, np.concatenate((set_masks(cut, O, a), set_masks(n - cut, O, b))), what)
                else:
                    tn, tp = w.step(what, lambda: ctx.calculateOutputTopK(32), n, "dense", ("out",))
                    check_topk(net, r, tn, tp, 32, what)
            check_hidden(net, r, ctx.hiddenActivations(), f"e n = {n}, after every output kind")
    finally:
        s.close()


# --------------------------------------------------------------------------------------------------- f. a seeded walk
WALK_SIZES = {"n256": (1, 31, 32, 33, 64, 65, 127, 128, 129, 256, 257, 320, 321, 511, 512, 513, 640, 641, 1025), "full": (1, 65, 321, 513, 641, 1025)}
WALK_ENTRIES = ("dense", "byte masks", "bit masks", "lists", "set", "top-k")


@pytest.mark.parametrize("seed", [11, 12])
@pytest.mark.parametrize("name,steps", [("n256", 24), ("full", 8)])
def test_f_seeded_walk_over_entries_sizes_and_modes(nets, query, name, steps, seed):
    net = nets(name)
    O = net.O
    rng = np.random.default_rng(seed * 1000 + steps)
    s = Streamed(net, max(WALK_SIZES[name]))
    w = Walk(net, query, ctx_audit(s.view))
    try:
        for i in range(steps):
            n = int(rng.choice(WALK_SIZES[name]))
            kind = WALK_ENTRIES[int(rng.integers(len(WALK_ENTRIES)))]
            fuse, chain, ppo, l0k = int(rng.integers(2)), int(rng.integers(2)), int(rng.integers(-1, 2)), int(rng.choice((0, 1, 2, 4)))
            what = f"f{i} {kind}, n = {n}, fuse {fuse} chain {chain} ppo {ppo} layer-0 kernel {l0k}"
            r = net.ref(n)
            ctx = w.step(what + ": hidden layers", lambda: s.hidden(n), n, "none", ("l0", "hid"), fuse=fuse, chain=chain, ppo=ppo, l0k=l0k)
            check_hidden(net, r, ctx.hiddenActivations(), what)
            masks = masks_for(n, O, seed=90 + n)
            rp, nd = F.masks_to_lists(masks)
            nodes = LS.pick(O, min(70, O), 91 + n, (0, O - 1))
            m = dict(fuse=fuse, chain=chain, ppo=ppo, l0k=l0k)
            if kind == "dense":
                check_dense(net, r, w.step(what, ctx.calculateOutput, n, "dense", ("out",), **m), what)
            elif kind == "byte masks":
                check_lazy(net, r, w.step(what, lambda: ctx.calculateForOutputNodesBatch(masks), n, "bytes", ("out",), **m), masks, what)
            elif kind == "bit masks":
                check_lazy(net, r, w.step(what, lambda: ctx.calculateForOutputNodesBatchBits(F.pack_mask_bits(masks)), n, "bits", ("out",), **m), masks, what)
            elif kind == "lists":
                probs, inactive = w.step(what, lambda: ctx.calculateForOutputNodesLists(rp, nd), n, "none", (), **m)
                check_lazy(net, r, rows_of_lists(rp, nd, probs, inactive, masks, O), masks, what)
            elif kind == "set":
                probs, inactive = w.step(what, lambda: ctx.calculateForOutputNodeSet(nodes), n, "none", (), **m)
                check_lazy(net, r, rows_of_set(nodes, probs, inactive, O), set_masks(n, O, nodes), what)
            else:
                k = min(32, O)
                tn, tp = w.step(what, lambda: ctx.calculateOutputTopK(k), n, "dense", ("out",), **m)
                check_topk(net, r, tn, tp, k, what)
    except AssertionError:
        print("the walk so far:", *w.trace, sep="\n  ")
        raise
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ g. the scoring loop's slots
def test_g_scoring_loop_slots_are_clean_at_teardown(nets):
    net = nets("mid")
    dnn, O = net.dnn, net.O
    depth = 2
    before = net.counters()
    api.scratch_dirty()
    api.scratch_audit(True)
    srv = api.ScoringServer(dnn, 512, depth)
    try:
        jobs = []
        for j, (kind, n) in enumerate((("dense", 100), ("lazy", 37), ("set", 64), ("top-k", 200), ("dense", 1), ("lazy", 300), ("top-k", 33), ("set", 129),
                                       ("dense", 512))):
            r = net.ref(n)
            masks = masks_for(n, O, seed=120 + j)
            nodes = LS.pick(O, 70, 130 + j, (0, O - 1))
            if kind == "dense":
                t, out = srv.submit(r["x"])
                jobs.append((t, kind, n, r, lambda out=out: out, None))
            elif kind == "lazy":
                t, out = srv.submitLazy(r["x"], F.pack_mask_bits(masks))
                jobs.append((t, kind, n, r, lambda out=out: out, masks))
            elif kind == "set":
                t, probs, inactive = srv.submitLazySet(r["x"], nodes)
                jobs.append((t, kind, n, r, lambda probs=probs, inactive=inactive, nodes=nodes: rows_of_set(nodes, probs.reshape(-1, nodes.size), inactive, O),
                             set_masks(n, O, nodes)))
            else:
                t, tn, tp = srv.submitTopK(r["x"], 16)
                jobs.append((t, kind, n, r, lambda tn=tn, tp=tp: (tn, tp), None))
        for t, *_ in jobs:
            srv.wait(t)
    finally:
        srv.close()
    totals = DL.ScratchSpan.stop()
    DL.check_audit("the scoring loop's slots at teardown", totals, min_contexts=depth)
    assert net.counters() == before, f"fault counters moved: {before} -> {net.counters()}"
    for t, kind, n, r, result, masks in jobs:
        what = f"g {kind} n = {n}"
        if kind == "dense":
            check_dense(net, r, result(), what)
        elif kind == "top-k":
            check_topk(net, r, *result(), 16, what)
        else:
            check_lazy(net, r, result(), masks, what)
