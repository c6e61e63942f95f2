"""One context, the four alignment families, sizes that move.  align, alignGraph, forwardBackward and
fbFrames share one context's staging buffers (fdnn_runtime.cpp: d_al_int, d_ag_int, d_ag_lp, d_al_probs, d_al_inact, d_al_bp,
d_fb_res, d_fb_int, d_fb_lp) under three layouts -- d_fb_res is total | gamma for one family and frame_total | alpha_out |
alpha_in for another, d_al_bp is back-pointers for one and an fp32 lattice for the others, the start_lp / final_lp tail of
d_ag_lp is skipped when the graph has none -- and a pooled production context serves all of them at sizes that shrink and
grow.  Every step of a walk on ONE LazyContext is held to the composed restatement (the bytes of the lazy sets call of the
MODEL, a pooled context of its own, through api.align_ref / align_graph_ref / fb_ref / fb_frames_ref), never to the library's
own earlier answer; the interleaved set, top-k and score steps to the oracle.  After every step the context's scratch audit
is clean and the model's fault counters stand where they stood; a failure names the step and its predecessor.  Across
consecutive steps of one family the EXPECTED results differ in bytes, so a step that returned its predecessor's leftover
would fail."""
import numpy as np
import pytest

import align_cases as AC
import align_graph_cases as GC
import dispatch_ledger as DL
import lazy_set_cases as LS
import loglik_cases as LL
import test_gpu_fb as FB
import test_gpu_fb_frames as FR
from fast_dnn_amd import api, formats as F
from oracle.oracle import Oracle
from test_gpu_ctx_sequences import NAMES, check_dense, check_lazy, check_topk, rows_of_set, set_masks

pytestmark = pytest.mark.gpu
N = 120
HANDLES = ((-np.inf, api.LOGLIK_F32), (-20.0, api.LOGLIK_F16))  # no floor, fp32; a floor, fp16


def eight_states(dense, seed):
    """An optional-silence transcript of a two-state and a three-state word: 8 states, arc scores ln U(0.05, 0.95); the
    words' nodes are drawn from the twelve nodes of the largest mean probability beside the silence, so the scores take part."""
    rng = np.random.default_rng(seed)
    sil = GC.silence_node(dense)
    best = [int(v) for v in np.argsort(-dense.mean(axis=0, dtype=np.float64), kind="stable") if v != sil][:12]
    nodes = [best[int(i)] for i in rng.integers(0, len(best), 5)]
    g = api.optional_silence_graph([nodes[:2], nodes[2:]], sil)
    assert len(g["states"]) == 8
    g["arc_lp"] = np.log(rng.uniform(0.05, 0.95, g["arc_lp"].size)).astype(np.float32)
    return g


class Net:
    def __init__(self, path, seed):
        self.dnn, self.orc = api.QuantizedDnn.loadFromFile(path, device=0), Oracle(path)
        self.O = self.dnn.outputDimension()
        self.x = F.synth_features(N, 432, seed=seed)
        with np.errstate(all="ignore"):
            hid = self.orc.hidden_acts_mt(self.x)
            want, acc = self.orc.output_mt(hid, want_acc=True)
        self.r = dict(x=self.x, idx=np.arange(N), hid=hid, want=want, acc=acc)
        self.dense = self.dnn.calculate(self.x)
        self.lp = LL.priors(self.O)
        one, three = np.array([0, N], np.int32), np.array([0, 37, 81, N], np.int32)
        big = GC.silence_graphs(self.dense, three, 3, words_per_seg=50)  # 3 x 201 states, 3 x about 600 arcs
        rng = np.random.default_rng(seed)
        for g in big:  # entered and left anywhere: 201 states have a path over 40 frames
            g["start_lp"] = np.log(rng.uniform(0.05, 0.95, len(g["states"]))).astype(np.float32)
            g["final_lp"] = np.log(rng.uniform(0.05, 0.95, len(g["states"]))).astype(np.float32)
        bare = lambda g: dict(g, start_lp=None, final_lp=None)
        self.graphs = {"small": (one, api.pack_graphs([eight_states(self.dense, 1)])),
                       "small2": (one, api.pack_graphs([eight_states(self.dense, 2)])),
                       "big": (three, api.pack_graphs(big)),
                       "bare more arcs": (one, api.pack_graphs([bare(g) for g in GC.silence_graphs(self.dense, one, 4, words_per_seg=9)])),
                       "bare fewer arcs": (one, api.pack_graphs([bare(eight_states(self.dense, 5))]))}
        self.carry = {k: np.random.default_rng(9).uniform(-30, -5, int(p["statePtr"][-1])).astype(np.float32) for k, (_, p) in self.graphs.items()}
        self.transcripts = {}
        for k, segs in (("one", one), ("three", three)):
            ptr, states = AC.transcripts(self.dense, segs, 6 + len(k))
            self.transcripts[k] = (segs, ptr, states) + AC.transitions(states.size, 7)

    def counters(self):
        return self.dnn.chainFaults(), int(self.dnn.deviceCounters(4)[3]), self.dnn.fuseGiveups()

    def close(self):
        self.dnn.delete()
        self.orc.close()


@pytest.fixture(scope="module")
def nets(tiny_model_path):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Net(tiny_model_path if name == "tiny" else DL.net_path("n256/256/gauss"), 2700 + len(name))
        return cache[name]

    yield get
    for net in cache.values():
        net.close()


def bits(parts):
    return tuple(None if p is None else np.ascontiguousarray(p).view(np.uint32 if p.dtype.itemsize == 4 else np.uint16).tobytes() for p in parts)


class Walk:
    def __init__(self, net, torch):
        self.net, self.torch = net, torch
        self.ctx = net.dnn.getNewLazyContext(N)
        self.ctx.calculateUntilOutput(net.x)
        self.lls = [api.Loglik(net.lp, *h) for h in HANDLES]
        self.st = torch.cuda.Stream()
        self.prev, self.trace, self.last_want = "(a fresh context)", [], {}

    def close(self):
        api.set_fb_kernel(0)
        for ll in self.lls:
            ll.delete()
        self.ctx.delete()

    def dev(self, n, dtype=None):
        return self.torch.full((max(n, 1),), -7, dtype=dtype or self.torch.float32, device="cuda")

    def run(self, kind, arg, h, device):
        """-> (family, got, want): both tuples of arrays, compared as bytes."""
        net, ctx, ll, handle, st = self.net, self.ctx, self.lls[h], HANDLES[h], self.st
        if kind == "align":
            segs, ptr, states, sl, nl = net.transcripts[arg]
            want = AC.composed(net.dnn, net.x, net.lp, handle, segs, ptr, states, sl, nl)
            if device:
                d_path, d_total = self.dev(N, self.torch.int32), self.dev(segs.size - 1)
                ctx.alignDevice(ll, segs, ptr, states, d_path.data_ptr(), d_total.data_ptr(), sl, nl, st.cuda_stream)
                st.synchronize()
                return kind, (d_path.cpu().numpy(), d_total.cpu().numpy()), want
            return kind, ctx.align(ll, segs, ptr, states, sl, nl), want
        segs, packed = net.graphs[arg[0]] if kind != "sets" else (None, None)
        if kind == "graph":
            want = GC.composed(net.dnn, net.x, net.lp, handle, segs, packed)[0]
            if device:
                d_path, d_total = self.dev(N, self.torch.int32), self.dev(segs.size - 1)
                ctx.alignGraphDevice(ll, segs, packed, d_path.data_ptr(), d_total.data_ptr(), st.cuda_stream)
                st.synchronize()
                return kind, (d_path.cpu().numpy(), d_total.cpu().numpy()), want
            return kind, ctx.alignGraph(ll, segs, packed), want
        if kind == "fb":
            gamma = arg[1]
            want = FB.composed(net.dnn, net.x, net.lp, handle, segs, packed, want_gamma=gamma)
            if device:
                cells = int((np.diff(segs).astype(np.int64) * np.diff(packed["statePtr"])).sum())
                d_total, d_gamma = self.dev(segs.size - 1), self.dev(cells)
                ctx.forwardBackwardDevice(ll, segs, packed, d_total.data_ptr(), d_gamma.data_ptr() if gamma else 0, st.cuda_stream)
                st.synchronize()
                return kind, (d_total.cpu().numpy(), d_gamma.cpu().numpy()[:cells] if gamma else None), want
            return kind, ctx.forwardBackward(ll, segs, packed, gamma), want
        if kind == "frames":
            free, carry = arg[1], net.carry[arg[0]] if arg[2] else None
            want = FR.composed(net.dnn, net.x, net.lp, handle, segs, packed, free_start=free, alpha_in=carry)
            if device:
                d_tot, d_out = self.dev(N), self.dev(carry.size if carry is not None else int(packed["statePtr"][-1]))
                d_in = self.torch.from_numpy(carry).cuda() if carry is not None else None
                self.torch.cuda.synchronize()
                ctx.fbFramesDevice(ll, segs, packed, d_tot.data_ptr(), free, d_in.data_ptr() if carry is not None else 0, d_out.data_ptr(), st.cuda_stream)
                st.synchronize()
                return kind, (d_tot.cpu().numpy(), d_out.cpu().numpy()), want
            return kind, ctx.fbFrames(ll, segs, packed, free, carry), want
        raise AssertionError(kind)

    def step(self, label, kind, arg=None, h=0, mode=0, device=False):
        what = f"step '{label}' (after {self.prev})"
        self.trace.append(label)
        net = self.net
        before = net.counters()
        api.set_fb_kernel(mode)
        try:
            if kind == "sets":  # the interleaved steps, held to the oracle
                a, b = LS.pick(net.O, min(70, net.O), 71, (0, net.O - 1)), LS.pick(net.O, min(129, net.O), 72, (net.O - 1,))
                cut = 33
                probs, inactive = self.ctx.calculateForOutputNodeSets([0, cut, N], [0, a.size, a.size + b.size], np.concatenate((a, b)))
                rows = np.concatenate((rows_of_set(a, probs[:cut * a.size].reshape(cut, a.size), inactive[:cut], net.O),
                                       rows_of_set(b, probs[cut * a.size:].reshape(N - cut, b.size), inactive[cut:], net.O)))
                check_lazy(net, net.r, rows, np.concatenate((set_masks(cut, net.O, a), set_masks(N - cut, net.O, b))), what)
            elif kind == "topk":
                k = min(32, net.O)
                check_topk(net, net.r, *self.ctx.calculateOutputTopK(k), k, what)
            elif kind == "loglik":
                got = self.ctx.calculateOutputLoglik(self.lls[h])
                assert LL.same_bytes(got, api.loglik_ref(net.dense, net.lp, *HANDLES[h])), f"{what}: not the scores of the dense rows the oracle holds"
            else:
                family, got, want = self.run(kind, arg, h, device)
                g, w = bits(got), bits(want)
                assert g == w, f"{what}: not the composed restatement's bytes (parts that differ: {[i for i, (x, y) in enumerate(zip(g, w)) if x != y]})"
                # not blind: a step that returned its predecessor's leftover would fail
                assert self.last_want.get(family) != w, f"{what}: the restatement expects the bytes of the {family} step before it"
                self.last_want[family] = w
        finally:
            api.set_fb_kernel(0)
        state = self.ctx.scratchState()
        dirty = {k: v for k, v in state.items() if k in NAMES and v}
        assert not dirty, f"{what}: scratch audit: counters left non-zero (buffer: words) {dirty}; sequence so far: {self.trace}"
        assert net.counters() == before, f"{what}: fault counters moved: {before} -> {net.counters()}"
        self.prev = f"'{label}'"


# label, kind, argument, handle, fb kernel mode, device form -- and the transition the step is there for
LITERAL = (
    ("1 fbFrames anchored, 1 x 8 states", "frames", ("small", False, False), 0, 0, False),       # every shared buffer small ..
    ("2 forwardBackward with gamma, 3 x 201 states", "fb", ("big", True), 0, 0, False),           # .. grown ..
    ("3 fbFrames free, 3 x 201 states", "frames", ("big", True, False), 0, 0, False),             # .. (d_fb_res in its other layout, grown)
    ("4 alignGraph, 3 x 201 states", "graph", ("big",), 0, 0, False),
    ("5 fbFrames anchored, 1 x 8 states again", "frames", ("small2", False, False), 0, 0, False),  # .. and reused smaller
    ("6 align, three segments", "align", "three", 0, 0, False),                                   # d_al_bp: int back-pointers ..
    ("7 fbFrames free behind align", "frames", ("big", True, False), 1, 0, False),                # .. then read as a lattice; a handle change: F32 without a floor -> F16 with one
    ("8 align, one segment", "align", "one", 1, 0, False),
    ("9 forwardBackward with gamma behind align", "fb", ("small", True), 1, 0, False),            # back-pointers, then the lattice; total | gamma ..
    ("10 fbFrames free with a carried row", "frames", ("small", True, True), 1, 0, False),        # .. then frame_total | alpha_out | alpha_in
    ("11 forwardBackward with gamma", "fb", ("small2", True), 0, 0, False),
    ("12 forwardBackward without gamma", "fb", ("big", False), 0, 0, False),                      # .. directly behind gamma: no lattice, no gamma words
    ("13 lazy sets", "sets", None, 0, 0, False),
    ("14 fbFrames, graph with start_lp and final_lp", "frames", ("small", True, False), 0, 0, False),
    ("15 fbFrames, more arcs, neither", "frames", ("bare more arcs", True, False), 0, 0, False),  # the tail of d_ag_lp is stale ..
    ("16 fbFrames, fewer arcs, neither", "frames", ("bare fewer arcs", True, False), 0, 0, False),  # .. and lies where the larger graph's arcs were
    ("17 top-k", "topk", None, 0, 0, False),
    ("18 fbFrames free, wave form forced", "frames", ("big", True, True), 0, 1, False),           # modes 1, 2, 0 on identical arguments
    ("19 the same, workgroup form forced", "frames", ("big", True, True), 0, 2, False),
    ("20 the same under the rule", "frames", ("big", True, True), 0, 0, False),
    ("21 scores", "loglik", None, 1, 0, False),
    ("22 fbFramesDevice on a side stream, carried", "frames", ("small", True, True), 1, 0, True),
    ("23 forwardBackwardDevice with gamma", "fb", ("big", True), 1, 0, True),
    ("24 alignGraphDevice", "graph", ("small",), 1, 0, True),
    ("25 alignDevice", "align", "three", 1, 0, True),
)
SAME_ARGUMENTS = {"19 the same, workgroup form forced", "20 the same under the rule"}  # (the blindness condition cannot hold between them)


def walk(net, torch, steps):
    before = net.dnn.calculate(net.x)
    check_dense(net, net.r, before, "before the walk")
    w = Walk(net, torch)
    try:
        for label, kind, arg, h, mode, device in steps:
            if label in SAME_ARGUMENTS:
                w.last_want.pop(kind, None)
            w.step(label, kind, arg, h, mode, device)
    except AssertionError:
        print("the walk so far:", *w.trace, sep="\n  ")
        raise
    finally:
        w.close()
    assert np.array_equal(net.dnn.calculate(net.x).view(np.uint32), before.view(np.uint32)), "the dense entry point's bytes moved over the walk"


@pytest.mark.parametrize("name", ("n256", "tiny"))
def test_a_literal_sequence_over_the_four_families(nets, name):
    import torch

    walk(nets(name), torch, LITERAL)


@pytest.mark.parametrize("name", ("n256", "tiny"))
def test_a_seeded_walk_over_the_four_families(nets, name):
    import torch

    rng = np.random.default_rng(31 + len(name))
    graphs = ("small", "small2", "big", "bare more arcs", "bare fewer arcs")
    steps, last = [], {}
    while len(steps) < 24:
        kind = ("align", "graph", "fb", "frames", "sets", "topk", "loglik")[int(rng.choice(7, p=(0.15, 0.15, 0.2, 0.3, 0.07, 0.07, 0.06)))]
        g = graphs[int(rng.integers(len(graphs)))]
        arg = {"align": ("one", "three")[int(rng.integers(2))], "graph": (g,), "fb": (g, bool(rng.integers(2))),
               "frames": (g, bool(rng.integers(2)), bool(rng.integers(2)))}.get(kind)
        h, mode, device = int(rng.integers(2)), int(rng.integers(3)), bool(rng.integers(2)) and kind in ("align", "graph", "fb", "frames")
        key = (arg, h)
        if kind in last and last[kind] == key:
            continue  # (the same arguments as the family's step before: the blindness condition could not hold)
        if kind in ("align", "graph", "fb", "frames"):
            last[kind] = key
        steps.append((f"w{len(steps)} {kind} {arg} handle {h} mode {mode}{' device' if device else ''}", kind, arg, h, mode, device))
    walk(nets(name), torch, steps)
