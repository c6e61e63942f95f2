"""Every pass held to the oracle at the limits of the nets the loader accepts (read_raw_model, fdnn_model.cpp).

  A  depth         2 .. 29 int8 hidden layers (31 affine layers): the tap buffers' layer stride, a launch per layer, and the
                   chained launches of at most 8 layers each -- 9 layers run as 8 + 1, 16 as 8 + 8, 17 as 8 + 8 + 1, 29 as
                   8 + 8 + 8 + 5, sharing one set of counters and carrying the ping-pong buffer from launch to launch
  B  output width  65 536 / 65 537 (the union path's last width and the first it refuses), 131 075, 2^19 = 524 288 (2048
                   soft-max tiles: normalize_row's whole tree)
  C  hidden width  K = 4112: accumulators beyond 2^26 in magnitude, which the load-time division sweep used to leave out
  D  input width   either side of the layer-0 rules' edges: the int8 screening (D <= 496), the small kernel's LDS (596 / 600;
                   608, 612 and 616 lie above it), the fp32 screening's LDS (D <= 4096)

The nets come from tests/limit_nets.py; tests/test_limit_nets_host.py asserts on the CPU that they are not degenerate.
Every comparison is with the oracle (never with another library path, except where a case ALSO asks for equal bytes from
two forms); integers and bytes are compared for equality, soft-max rows by the ledger's checks.  Every case runs under the
launch recorder and asserts the instance names it is about."""
import math

import numpy as np
import pytest

import limit_nets as LN
import topk_cases as TK
from dispatch_ledger import TIGHT, _masked_out_ok, _softmax_ok, _softmax_rel_ok
from fast_dnn_amd import api, formats as F
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

HOT = 2e-4         # tools/fuzz_parity.py's arm for w_std > 0.05: the reference's own sequential fp32 row sum is the inexact side
NORTH_STAR = 1e-3  # README: the bar on |p - reference|


# ------------------------------------------------------------------------------------------------------------ plumbing
def recorded(fn, *args, **kwargs):
    """fn(...) with the recorder on -> (its result, {name: launches})."""
    api.launch_record(True)
    api.launch_reset()
    try:
        res = fn(*args, **kwargs)
        return res, dict(api.launch_counts())
    finally:
        api.launch_record(False)


@pytest.fixture()
def modes():
    yield
    api.set_fuse(-1)
    api.set_chain(-1)
    api.set_pp(-1)
    api.set_ppo(-1)
    api.set_kernel(0)


_NETS = {}


@pytest.fixture(scope="module")
def nets(tmp_models):
    """get(name, topology, make) -> dict(path, dnn, orc), loaded once per module."""
    def get(name, topology, make):
        if name not in _NETS:
            path = LN.cached(tmp_models, name, topology, make)
            _NETS[name] = dict(path=path, dnn=api.QuantizedDnn.loadFromFile(path, device=0), orc=Oracle(path))
        return _NETS[name]

    yield get
    for m in _NETS.values():
        m["dnn"].delete()
        m["orc"].close()
    _NETS.clear()
    _REF.clear()  # (the wide cases' references are hundreds of megabytes: not kept for the rest of the session)


@pytest.fixture()
def l0_kind():
    """set(dnn, kind): force a model's layer-0 kernel; the default rule is back at teardown."""
    touched = []

    def force(dnn, kind):
        touched.append(dnn)
        dnn.setInputLayerKernel(kind)

    yield force
    for dnn in touched:
        dnn.setInputLayerKernel(0)


@pytest.fixture()
def lists_union():
    """set(dnn, group_tiles): fdnn_model_set_lists_union; off again at teardown."""
    touched = []

    def switch(dnn, group_tiles):
        touched.append(dnn)
        dnn.setListsUnion(group_tiles)

    yield switch
    for dnn in touched:
        dnn.setListsUnion(0)


_REF = {}


def reference(key, orc, x):
    """The oracle's (probabilities, taps) of a batch, computed once per key -- (group, ...) -- and left unchanged."""
    if key not in _REF:
        want, wt = LN.taps_mt(orc, x)
        for a in (want, *[v for v in wt.values() if isinstance(v, np.ndarray)]):
            a.setflags(write=False)
        _REF[key] = (want, wt)
    return _REF[key]


def hidden_bytes(dnn, x, ctx=None):
    own = ctx is None
    if own:
        ctx = dnn.getNewLazyContext(x.shape[0])
    ctx.calculateUntilOutput(x)
    got = ctx.hiddenActivations().copy()
    if own:
        ctx.delete()
    return got


def abs_err(got, want):
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern differs from the oracle"
    return float(np.nanmax(np.abs(got - want))) if got.size else 0.0


def hot_softmax_ok(got, want, orc, acc, what, masks=None):
    """_softmax_rel_ok, and the absolute bar by tools/fuzz_parity.py's rule: these nets have w_std 0.3 / 0.5, its 2e-4 arm."""
    _softmax_rel_ok(got, want, orc, acc, what, masks=masks)
    err = abs_err(got, want)
    print(f"{what}: |p - oracle| {err:.3e} ({'within the 2e-6 arm too' if err <= TIGHT else 'the 2e-4 arm is the one that holds'})")
    assert err <= HOT, f"{what}: soft-max differs from the oracle by {err:.3e} (> {HOT})"


# ============================================================================================================= A. depth
DEPTHS = LN.DEPTHS
DEPTH_IDS = [f"hid{d}" for d, _ in DEPTHS]


def deep(nets, n_hid, w_std, width=256):
    return nets(f"limit_deep_{n_hid}x{width}", LN.deep_topology(n_hid, width), lambda: LN.deep_net(n_hid, width, w_std=w_std))


def deep_x(n):
    return F.synth_features(n, 432, seed=3000 + n % 977)


@pytest.mark.parametrize("n", (33, 1409))
@pytest.mark.parametrize("n_hid,w_std", DEPTHS, ids=DEPTH_IDS)
def test_depth_taps(nets, n_hid, w_std, n):
    """forwardTaps: the bytes of EVERY layer and every accumulator are the oracle's (the tap buffers' layer stride at depth 30)."""
    m = deep(nets, n_hid, w_std)
    x = deep_x(n)
    want, wt = reference(("deep", n_hid, n), m["orc"], x)
    got, ran = recorded(m["dnn"].forwardTaps, x)
    must = {33: "small.hid.nt32.tap", 1409: "gemm.hid.ft32.w1.tap"}[n]
    assert ran.get(must, 0) == n_hid, f"{must} x {n_hid} expected; launched {ran}"
    assert got["u8_acts"].shape == (n_hid + 1, n, 256) and got["acc_hid"].shape == (n_hid, n, 256)
    for li in range(n_hid + 1):
        assert np.array_equal(got["u8_acts"][li], wt["u8_acts"][li]), f"hidden layer {li}: bytes differ from the oracle"
    for li in range(n_hid):
        assert np.array_equal(got["acc_hid"][li], wt["acc_hid"][li]), f"int8 hidden layer {li}: accumulators differ from the oracle"
    assert np.array_equal(got["acc_out"], wt["acc_out"])


@pytest.mark.parametrize("n", (33, 1409))
@pytest.mark.parametrize("n_hid,w_std", DEPTHS, ids=DEPTH_IDS)
def test_depth_one_launch_per_layer(nets, modes, n_hid, w_std, n):
    """set_chain(0): the production instances, dense and lazy soft-max.  Absolute arm used: 2e-4 (hot weights; the measured
    error is printed, and where it is below 2e-6 the print says so)."""
    m = deep(nets, n_hid, w_std)
    dnn, orc = m["dnn"], m["orc"]
    x = deep_x(n)
    want, wt = reference(("deep", n_hid, n), orc, x)
    api.set_chain(0)
    hid, ran = recorded(hidden_bytes, dnn, x)
    must = {33: "small.hid.nt32.prod", 1409: "gemm.hid.ft32.w1.prod"}[n]
    assert ran.get(must, 0) == n_hid and not any(k.startswith("chain.") for k in ran), f"{must} x {n_hid} expected; launched {ran}"
    assert np.array_equal(hid, wt["u8_acts"][-1]), "last hidden layer's bytes differ from the oracle"
    what = f"depth {n_hid}, n {n}"
    hot_softmax_ok(dnn.calculate(x), want, orc, wt["acc_out"], what + " dense")
    masks = F.generate_masks(n, orc.out_dim, 0.40, 0.03, seed=7 + n_hid)
    lazy = dnn.calculateLazy(x, masks=masks)
    hot_softmax_ok(lazy, orc.output_mt(wt["u8_acts"][-1], masks=masks), orc, wt["acc_out"], what + " lazy", masks=masks)
    _masked_out_ok(lazy, masks, what)


def chain_rows(n, T, seed):
    """The frames the oracle scores of a chained pass: in-tile rows 0, 31, 32, T - 1 of the first, a middle and the last
    tile, frame n - 1, and 64 random frames."""
    tiles = -(-n // T)
    pick = {n - 1}
    for t in {0, tiles // 2, tiles - 1}:
        pick.update(f for f in (t * T + r for r in (0, 31, 32, T - 1)) if f < n)
    rng = np.random.default_rng(seed)
    target = len(pick) + 64
    while len(pick) < target:
        pick.add(int(rng.integers(0, n)))
    return np.array(sorted(pick))


def chained_case(m, n_hid, n, T, K_name):
    """One forced-chain pass and two more on the same context against the oracle on chain_rows and against the per-layer form."""
    dnn, orc = m["dnn"], m["orc"]
    x = deep_x(n)
    idx = chain_rows(n, T, seed=n + n_hid)
    want_hid = orc.hidden_acts_mt(x[idx])
    LN.assert_keeps_signal(want_hid, f"{K_name} depth {n_hid}")
    api.set_chain(0)
    per_layer, ran = recorded(hidden_bytes, dnn, x)
    assert not any(k.startswith("chain.") for k in ran), ran
    assert np.array_equal(per_layer[idx], want_hid), "per-layer form: last hidden layer's bytes differ from the oracle"
    api.set_chain(1, 1)
    ctx = dnn.getNewLazyContext(n)
    try:
        for turn in range(3):  # a counter left dirty by the last launch of a pass shows in the next pass
            got, ran = recorded(hidden_bytes, dnn, x, ctx)
            chains = {k: v for k, v in ran.items() if k.startswith("chain.")}
            assert chains and all(k.startswith(f"chain.ft{T}.") for k in chains), f"turn {turn}: chain.ft{T}.* expected; launched {ran}"
            assert not any(k.startswith(("gemm.hid.", "small.hid.", "pp.hid.")) for k in ran), f"turn {turn}: a per-layer instance ran: {ran}"
            assert sum(chains.values()) == math.ceil(n_hid / 8), f"turn {turn}: {chains}: {math.ceil(n_hid / 8)} chained launches expected"
            assert dnn.deviceCounters(8)[3] == 0, f"turn {turn}: a wait of the chained kernel ran into its bound"
            assert np.array_equal(got[idx], want_hid), f"turn {turn}: last hidden layer's bytes differ from the oracle"
            assert np.array_equal(got, per_layer), f"turn {turn}: bytes differ from the per-layer form"
    finally:
        ctx.delete()


@pytest.mark.parametrize("n,T", ((641, 256), (1281, 320)))
@pytest.mark.parametrize("n_hid,w_std", DEPTHS, ids=DEPTH_IDS)
def test_depth_chained(nets, modes, n_hid, w_std, n, T):
    """set_chain(1, 1): ceil(n_hid / 8) chained launches (1, 1, 1, 2, 2, 3, 4 for 2 .. 29 layers), no launch per layer."""
    chained_case(deep(nets, n_hid, w_std), n_hid, n, T, "K 256")


def test_depth_chained_8_plus_1_at_production_k(nets, modes):
    """[432] + [2048] * 10 + [252]: nine int8 hidden layers on the chained kernel's own shape, a launch of 8 and a launch of ONE."""
    chained_case(deep(nets, 9, 0.3, width=2048), 9, 641, 256, "K 2048")


def test_depth_29_scoring_loop(nets):
    """Dense and masked submissions through the scoring loop, coalesced into shared batches, are bit-identical to the calls."""
    m = deep(nets, 29, 0.3)
    dnn, orc = m["dnn"], m["orc"]
    xs = [deep_x(n) for n in (100, 37, 250, 64)]
    masks = {1: F.generate_masks(37, orc.out_dim, seed=1), 3: F.generate_masks(64, orc.out_dim, seed=2)}
    want, acc = orc.output_mt(orc.hidden_acts_mt(xs[2]), want_acc=True)
    alone = [dnn.calculateLazy(x, masks=masks[i]) if i in masks else dnn.calculate(x) for i, x in enumerate(xs)]
    hot_softmax_ok(alone[2], want, orc, acc, "depth 29, the call")
    srv = api.ScoringServer(dnn, 512, 2, linger_us=2000)
    try:
        tickets = [srv.submit(x, masks=masks.get(i)) for _ in range(3) for i, x in enumerate(xs)]
        for t, _ in tickets:
            srv.wait(t)
        for j, (_, out) in enumerate(tickets):
            assert np.array_equal(out.view(np.uint32), alone[j % 4].view(np.uint32)), f"submission {j} differs from the call"
        st = srv.stats()
        print("scoring loop at depth 29:", st)
        assert st["requests"] == 12 and st["coalesced_requests"] > 0 and st["batches"] < st["requests"], st  # submissions really shared batches
    finally:
        srv.close()


def test_depth_29_blob_round_trip(nets):
    import torch

    m = deep(nets, 29, 0.3)
    x = deep_x(33)
    _, wt = reference(("deep", 29, 33), m["orc"], x)
    nbytes = m["dnn"].blobSize()
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    m["dnn"].exportBlob(buf.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    info = api.host_blob_check(buf.cpu().numpy())
    assert info == dict(input_dim=432, hidden_dim=256, output_dim=252, n_affine=31)
    twin = api.QuantizedDnn.fromDeviceBlob(buf.data_ptr(), nbytes, 0)
    try:
        got = twin.forwardTaps(x)
        for k in ("u8_acts", "acc_hid", "acc_out"):
            assert np.array_equal(got[k], wt[k]), f"imported blob: {k} differs from the oracle"
        assert np.array_equal(twin.calculate(x).view(np.uint32), m["dnn"].calculate(x).view(np.uint32))
    finally:
        twin.delete()


def test_depth_29_float_net(nets):
    """FloatDnn: every one of the 31 layers against fdnn_debug_float_layer_ref, as test_gpu_float.py::test_tiny_every_layer."""
    from test_gpu_float import chain

    m = deep(nets, 29, 0.3)
    net = F.read_model_bin(m["path"])
    fdnn = api.FloatDnn.loadFromFile(m["path"], device=0)
    try:
        assert fdnn.layerCount() == 31
        x = deep_x(129)
        before = api.float_launches()
        got, _ = chain(fdnn, net, x, "depth 29, float net")
        assert np.array_equal(fdnn.calculate(x).view(np.uint32), got.view(np.uint32))
        after = api.float_launches()
        assert after["fgemm.sigmoid.tap"] - before["fgemm.sigmoid.tap"] == 30 and after["fgemm.exp.tap"] - before["fgemm.exp.tap"] == 1
        assert after["fgemm.sigmoid"] - before["fgemm.sigmoid"] == 30 and after["fgemm.exp"] - before["fgemm.exp"] == 1
    finally:
        fdnn.delete()


# ====================================================================================================== B. output width
# (W, n) -> the output and normalise instances a dense production pass launches, as observed on an MI355X: a later change
# of rule shows here.  K = 16 <= 2048 and n <= 512: the small-batch output kernel at every width.
# The ledger's missing single tile of gemm.out.ft128 is NOT covered here, and that is a decision about file size: the tile
# needs more than 256 node tiles behind rows too long for the small-batch kernel (K > 2048), i.e. wide_out_net(65537,
# hidden=2064), a 580 MB file, on which frame_tile's cost model answers 128 for a single frame tile.  This file's nets
# keep hidden = 16 (8 .. 34 MB), whose batches up to 512 frames all take small.out.*.
WIDE_CASES = [(W, n) for W in (65536, 65537, 131075) for n in (5, 33, 130)] + [(524288, 5), (524288, 33)]
EXPECT_OUT = {case: (["norm.rows", "small.out.prod"], ["norm.rows", "small.out.prod"]) for case in WIDE_CASES}


def wide(nets, W):
    return nets(f"limit_wide_out_{W}", LN.wide_out_topology(W), lambda: LN.wide_out_net(W))


def wide_x(W, n):
    return F.synth_features(n, 432, seed=W % 977 + n)


def out_names(ran):
    return {k for k in ran if k.startswith(("gemm.out.", "small.out.", "ppo.", "norm."))}


def wide_checks(got, want, orc, acc, what, masks=None):
    """The float64 bound is the test; the absolute difference from the oracle's fp32 rows is reported and held to 1e-3 only
    (at 2^19 nodes the oracle's own sequential row sum is off by 1.3e-4 relative)."""
    _softmax_rel_ok(got, want, orc, acc, what, masks=masks)
    err = abs_err(got, want)
    print(f"{what}: |p - oracle| {err:.3e}")
    assert err <= NORTH_STAR, f"{what}: {err:.3e}"
    if masks is not None:
        _masked_out_ok(got, masks, what)


@pytest.mark.parametrize("W,n", WIDE_CASES)
def test_wide_output_dense(nets, modes, W, n):
    """Measured on an MI355X: |p - oracle| 1.7e-8 at 65 536 nodes, 1.5e-8 .. 1.6e-8 at 65 537, 1.5e-8 .. 1.7e-8 at 131 075 and
    1.8e-8 .. 1.9e-8 at 524 288 (the largest probability of these ladders is ~3e-4, so 1.3e-4 relative shows as 4e-8 at
    the most); every entry inside softmax_ref's float64 bound.  Printed by every run."""
    m = wide(nets, W)
    dnn, orc = m["dnn"], m["orc"]
    x = wide_x(W, n)
    want, wt = reference(("wide", W, n), orc, x)
    (acc, probs), ran = recorded(dnn.productionOutputAcc, x, 1, probs=True)
    assert np.array_equal(acc, wt["acc_out"]), "output accumulators differ from the oracle"
    what = f"W {W}, n {n}"
    wide_checks(probs, want, orc, wt["acc_out"], what + " production")
    dense, ran2 = recorded(dnn.calculate, x)
    wide_checks(dense, want, orc, wt["acc_out"], what + " calculate")
    names = (sorted(out_names(ran)), sorted(out_names(ran2)))
    print(f"{what}: production pass {names[0]}, calculate {names[1]}")
    assert (W, n) in EXPECT_OUT and names == EXPECT_OUT[(W, n)], f"{what}: launched {names}, expected {EXPECT_OUT.get((W, n))}"
    for k in (1, 256):  # every width here is beyond TOPK_RESIDENT_WIDTH: the streaming form of the selection, never the resident one
        before = api.topk_launches()
        nodes, vals = dnn.calculateTopK(x, k)
        after = api.topk_launches()
        assert W > api.TOPK_RESIDENT_WIDTH and after[0] == before[0] and after[1] > before[1], f"{what}: top-{k} launches (resident, streaming) {before} -> {after}"
        wn, wv = TK.select(dense, k)
        assert np.array_equal(nodes, wn) and np.array_equal(vals.view(np.uint32), wv), f"{what}: top-{k} differs from the selection of the dense rows"


def rows_from(probs, inactive, nodes, W):
    out = np.repeat(np.asarray(inactive, np.float32)[:, None], W, axis=1)
    out[:, nodes] = probs
    return out


@pytest.mark.parametrize("W,n", WIDE_CASES)
def test_wide_output_lazy(nets, modes, lists_union, W, n):
    """Masks as bytes and as bits (5 % and 40 % active), lists on the dot-product kernels, one shared set of 80 nodes on the
    width's edges, two per-segment sets: each against the oracle's lazy rows."""
    m = wide(nets, W)
    dnn, orc = m["dnn"], m["orc"]
    x = wide_x(W, n)
    _, wt = reference(("wide", W, n), orc, x)
    hid, acc = wt["u8_acts"][-1], wt["acc_out"]
    gen = F.generate_masks_fast if n * W > (1 << 24) else F.generate_masks  # (the ledger's rule: the Python loop costs seconds there)
    ctx = dnn.getNewLazyContext(n)
    try:
        ctx.calculateUntilOutput(x)
        assert np.array_equal(ctx.hiddenActivations(), hid)
        for ratio in (0.05, 0.40):
            masks = gen(n, W, ratio, 0.03, seed=int(ratio * 100) + n)
            want = orc.output_mt(hid, masks=masks)
            for form in ("bytes", "bits"):
                got, ran = recorded(ctx.calculateForOutputNodesBatch, masks) if form == "bytes" else recorded(ctx.calculateForOutputNodesBatchBits, F.pack_mask_bits(masks))
                assert ran.get("small.out.masked", 0) == 1 and not any(k.startswith("gemm.out.") for k in ran), f"{form}: launched {ran}"
                wide_checks(got, want, orc, acc, f"W {W}, n {n}, {form} {ratio}", masks=masks)
            if ratio < 0.1:
                rp, nd = F.masks_to_lists(masks)
                before = api.lists_launches()
                probs, inactive = ctx.calculateForOutputNodesLists(rp, nd)
                assert sum(api.lists_launches()[:2]) > sum(before[:2]), "the dot-product list kernels did not run"
                wide_checks(F.lists_to_rows(rp, nd, probs, inactive, W), want, orc, acc, f"W {W}, n {n}, lists", masks=masks)
                # the union path: up to 65 536 nodes the bytes of the dot-product lists; beyond, refused, and the model stays usable
                lists_union(dnn, 2)
                ub = api.lists_union_launches()
                if W <= 65536:
                    up, ui = ctx.calculateForOutputNodesLists(rp, nd)
                    ua = api.lists_union_launches()
                    assert ua[0] > ub[0] and ua[1] + ua[2] > ub[1] + ub[2] and ua[3] == ub[3], (ub, ua)
                else:
                    with pytest.raises(api.FdnnError) as e:
                        ctx.listsUnion(rp, nd, 2)
                    assert e.value.code == api.FDNN_E_ARG and "65536" in str(e.value), str(e.value)
                    up, ui = ctx.calculateForOutputNodesLists(rp, nd)
                    ua = api.lists_union_launches()
                    assert ua[:3] == ub[:3] and ua[3] > ub[3], (ub, ua)  # (served by the dot-product kernels)
                assert np.array_equal(up.view(np.uint32), probs.view(np.uint32)) and np.array_equal(ui.view(np.uint32), inactive.view(np.uint32))
                lists_union(dnn, 0)
        nodes = LN.edge_nodes(W)
        set_mask = np.zeros((n, W), np.int8)
        set_mask[:, nodes] = 1
        # the MFMA set kernels themselves: run_set / run_sets hand a call to the list kernels, with the same bytes, where
        # set::shape_applies fails -- and one of its clauses, rows * ldw below the offset sentinel, depends on the width
        before = api.set_launches()
        sp, si = ctx.calculateForOutputNodeSet(nodes)
        after = api.set_launches()
        assert sum(after[:2]) == sum(before[:2]) + 1 and after[2] == before[2], f"W {W}: set launches (mfma, mfma + walk, by lists) {before} -> {after}"
        wide_checks(rows_from(sp, si, nodes, W), orc.output_mt(hid, masks=set_mask), orc, acc, f"W {W}, n {n}, shared set", masks=set_mask)
        other = LN.edge_nodes(W, count=200, seed=9)
        cut = n // 2
        seg_rows, set_ptr = [0, cut, n], [0, nodes.size, nodes.size + other.size]
        before = api.sets_launches()
        tp, ti = ctx.calculateForOutputNodeSets(seg_rows, set_ptr, np.concatenate((nodes, other)))
        after = api.sets_launches()
        assert sum(after[:2]) > sum(before[:2]) and after[2] == before[2], f"W {W}: sets launches (mfma, mfma + walk, by lists) {before} -> {after}"
        rp2, nd2 = F.sets_to_lists(seg_rows, set_ptr, np.concatenate((nodes, other)))
        set_mask[cut:] = 0
        set_mask[cut:, other] = 1
        wide_checks(F.lists_to_rows(rp2, nd2, tp, ti, W), orc.output_mt(hid, masks=set_mask), orc, acc, f"W {W}, n {n}, per-segment sets", masks=set_mask)
    finally:
        ctx.delete()
    assert np.array_equal(dnn.productionOutputAcc(x[:2], 1), acc[:2]), "the model is no longer usable"


# ====================================================================================================== C. hidden width
@pytest.fixture(scope="module")
def extreme(tmp_models):
    path, info = LN.extreme_acc_file(tmp_models)
    m = dict(path=path, info=info, dnn=api.QuantizedDnn.loadFromFile(path, device=0), orc=Oracle(path))
    yield m
    m["dnn"].delete()
    m["orc"].close()


def wide_hidden_case(m, n, key):
    """17 node tiles of 256: one-wave 32-frame tiles while they fit three rounds (33, 300 frames), the 128 x 128 shape at 1409."""
    must_tap, must_prod = (f"gemm.hid.{'ft32.w1' if n <= 300 else 'ft128.nt128'}.{b}" for b in ("tap", "prod"))
    dnn, orc = m["dnn"], m["orc"]
    x = F.synth_features(n, 432, seed=4000 + n)
    want, wt = reference(key, orc, x)
    got, ran = recorded(dnn.forwardTaps, x)
    assert not any(".tdiv." in k for k in ran) and ran.get(must_tap, 0) == 2, f"{must_tap} x 2 expected (validated division); launched {ran}"
    for k in ("u8_acts", "acc_hid", "acc_out"):
        assert np.array_equal(got[k], wt[k]), f"taps: {k} differs from the oracle"
    hid, ran = recorded(hidden_bytes, dnn, x)
    assert ran.get(must_prod, 0) == 2 and not any(".tdiv." in k for k in ran), f"{must_prod} x 2 expected; launched {ran}"
    assert np.array_equal(hid, wt["u8_acts"][-1]), "production: last hidden layer's bytes differ from the oracle"
    acc, probs = dnn.productionOutputAcc(x, 1, probs=True)
    assert np.array_equal(acc, wt["acc_out"])
    what = f"K 4112, n {n}"
    _softmax_ok(probs, want, what)
    _softmax_rel_ok(probs, want, orc, wt["acc_out"], what, tap=wt["logits"])
    return wt


@pytest.mark.parametrize("n", (33, 300, 1409))
def test_accumulators_beyond_2_26_divide_exactly(extreme, n):
    """K = 4112 > 2048: the tiled shapes from one frame up.  16 rows with |acc| in (2^26, 2056 * 32 768] whose quotients sit on
    table ties: one ulp of error in the division changes their byte."""
    wt = wide_hidden_case(extreme, n, ("acc", "planted", n))
    LN.assert_planted(extreme["info"], wt, extreme["orc"])


def test_plain_net_of_width_4112(nets):
    """The same net without the planted rows: K no multiple of 128 above 4096 on the ordinary shapes."""
    H = LN.ACC_H
    m = nets(f"limit_plain_{H}", [432, H, H, H, 252], lambda: LN.plain_wide_hidden_net(H))
    wide_hidden_case(m, 1409, ("acc", "plain", 1409))


# ======================================================================================================= D. input width
# (D, n, forced kind) -> the l0.* instances that ran, as observed on an MI355X (the widths and their edges: limit_nets.D_WIDTHS)
D_NS = (33, 128, 700, 2304)
_SCREEN, _SPLIT = ["l0.fix.tiles", "l0.screen.f128"], ["l0.digits", "l0.fixlist.lpo8", "l0.split.n64"]
_CHAIN12, _CHAIN16 = ["l0.chain.jc12.tn64.prod", "l0.image.frames"], ["l0.chain.jc16.tn64.prod", "l0.image.frames"]
EXPECT_L0 = {}  # D: (n 33, n 128, n 700, n 2304, n 2304 with the screening forced)
for _D, _row in {496: (["l0.small.prod"], ["l0.small.prod"], _SPLIT, _SPLIT, _SCREEN),
                 500: (["l0.small.prod"], ["l0.small.prod"], ["l0.tile32.prod"], ["l0.tile64.prod"], _SCREEN),
                 596: (["l0.small.prod"], ["l0.small.prod"], ["l0.tile32.prod"], ["l0.tile64.prod"], _SCREEN),
                 600: (["l0.tile16.prod"], ["l0.tile16.prod"], ["l0.tile32.prod"], ["l0.tile64.prod"], _SCREEN),
                 608: (["l0.tile16.prod"], ["l0.tile16.prod"], ["l0.tile32.prod"], ["l0.tile64.prod"], _SCREEN),
                 612: (["l0.tile16.prod"], ["l0.tile16.prod"], ["l0.tile32.prod"], ["l0.tile64.prod"], _SCREEN),
                 616: (["l0.tile16.prod"], ["l0.tile16.prod"], ["l0.tile32.prod"], ["l0.tile64.prod"], _SCREEN),
                 4096: (["l0.tile16.prod"], ["l0.tile16.prod"], _CHAIN16, ["l0.tile64.prod"], _SCREEN),
                 4100: (["l0.tile16.prod"], ["l0.tile16.prod"], _CHAIN12, ["l0.tile64.prod"], ["l0.tile64.prod"]),
                 8192: (["l0.tile16.prod"], ["l0.tile16.prod"], _CHAIN16, ["l0.tile64.prod"], ["l0.tile64.prod"])}.items():
    EXPECT_L0.update({(_D, 33, 0): _row[0], (_D, 128, 0): _row[1], (_D, 700, 0): _row[2], (_D, 2304, 0): _row[3], (_D, 2304, 3): _row[4]})


@pytest.mark.parametrize("D", LN.D_WIDTHS)
def test_input_width(nets, l0_kind, D):
    m = nets(f"limit_d_{D}", LN.d_topology(D), lambda: LN.d_net(D))
    dnn, orc = m["dnn"], m["orc"]
    seen, wrong = {}, []
    for n in D_NS:
        x = F.synth_features(n, D, seed=5000 + n, pad_from=None)
        want, wt = reference(("input", D, n), orc, x)
        for kind in ((0, 3) if n == 2304 else (0,)):
            l0_kind(dnn, kind)
            (u8, _), ran = recorded(dnn.layer0, x)
            names = sorted(k for k in ran if k.startswith("l0."))
            seen[(D, n, kind)] = names
            assert np.array_equal(u8, wt["u8_acts"][0]), f"D {D}, n {n}, kind {kind} ({names}): layer-0 bytes differ from the oracle"
            screened = any(k.startswith("l0.screen") for k in names)
            if kind == 3:
                assert screened == (D <= 4096), f"D {D}: forced screening launched {names}"
            if names != EXPECT_L0.get((D, n, kind)):
                wrong.append((D, n, kind))
            dense = dnn.calculate(x)
            what = f"D {D}, n {n}, kind {kind}"
            _softmax_ok(dense, want, what)
            _softmax_rel_ok(dense, want, orc, wt["acc_out"], what, tap=wt["logits"])
    print(f"D {D}: " + ", ".join(f"{k}: {v}" for k, v in seen.items()))
    assert not wrong, f"instances differ from EXPECT_L0 at {wrong}: " + repr({k: seen[k] for k in wrong})
