"""Lazy output by active-node lists (fdnn_ctx_lazy_output_lists / _device, fdnn_calculate_lazy_lists; fdnn_lists.hip) against the
oracle: the listed entries' int32 accumulators bit for bit (Oracle.output_mt(want_acc=True)), probabilities and inactive
values within 2e-6 of Oracle.lazy's rows, the three entry points byte-identical, and -- on the ladder net -- within the relative
bound of exp(z - max) / sum in float64.  The fixtures and their references: tests/lazy_lists_cases.py (the CPU file
tests/test_lazy_lists_host.py shows that the normative sum order itself meets these bars).

The relative bound (tests/softmax_ref.py's derivation with this path's summation):
    |got / p64 - 1| <= u (A_i + sum_j p_j A_j + DEPTH + 2),  A = 1.23 |z| + C_E_PATH["exp2.small"] for listed nodes, 0 for unlisted ones
    DEPTH = max(ceil(len / 64) - 1, 0) + 6 + 1   (a lane's chain, the butterfly's six levels, the unlisted nodes' term)"""
import threading

import numpy as np
import pytest

import lazy_lists_cases as LC
import softmax_ref as SR
from fast_dnn_amd import api, formats as F

pytestmark = pytest.mark.gpu
TIGHT = LC.TIGHT


@pytest.fixture(scope="module")
def fixtures(mid_model_path, sat_model_path, tiny_model_path, net_model_path):
    yield {"mid": mid_model_path, "sat": sat_model_path, "tiny": tiny_model_path, "full": net_model_path}
    LC.release()
    for d in _MODELS.values():
        d.delete()
    _MODELS.clear()


_MODELS = {}


def model(net, fixtures):
    if net not in _MODELS:
        _MODELS[net] = api.QuantizedDnn.loadFromFile(LC.model_path(net, fixtures))
    return _MODELS[net]


def device_form(dnn, x, row_ptr, nodes, first=0, count=None):
    """forward_hidden_device and the list call on ONE non-default stream, no synchronisation between them -> (probs, inactive)"""
    import torch

    n = x.shape[0]
    count = row_ptr.size - 1 if count is None else count
    nnz = int(row_ptr[-1])
    st = torch.cuda.Stream()
    dx = torch.from_numpy(x).cuda()
    drp, dnd = torch.from_numpy(row_ptr).cuda(), torch.from_numpy(np.concatenate((nodes, np.zeros(1, np.int32)))).cuda()
    dp = torch.full((nnz + 1,), -7.0, dtype=torch.float32, device="cuda")
    di = torch.full((count,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutputDevice(dx.data_ptr(), st.cuda_stream)
    ctx.calculateForOutputNodesListsDevice(drp.data_ptr(), dnd.data_ptr(), nnz, dp.data_ptr(), di.data_ptr(), first, count, st.cuda_stream)
    st.synchronize()
    probs, inactive = dp.cpu().numpy(), di.cpu().numpy()
    ctx.delete()
    assert probs[nnz] == -7.0  # nothing written past the entries
    return probs[:nnz], inactive


def same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", [c for c in LC.CASES if c not in LC.RELATIVE and not c.startswith("tail.")])
def test_lists_against_the_oracle_through_every_entry_point(fixtures, name):
    r = LC.reference(name, fixtures)
    net = LC.CASES[name][0]
    dnn = model(net, fixtures)
    x, row_ptr, nodes, n = r["x"], r["row_ptr"], r["nodes"], r["x"].shape[0]
    before = api.lists_launches()
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutput(x)
    acc = ctx.listsAccumulators(row_ptr, nodes)
    probs, inactive = ctx.calculateForOutputNodesLists(row_ptr, nodes)
    ctx.delete()
    after = api.lists_launches()
    assert np.array_equal(acc, r["acc"]), f"{name}: {int((acc != r['acc']).sum())} accumulators differ from the oracle"
    print(f"\n[lists] {name}: nnz {nodes.size}  max |p - oracle| {np.abs(probs - r['want_probs']).max(initial=0.0):.3e}", flush=True)
    assert np.abs(probs - r["want_probs"]).max(initial=0.0) <= TIGHT
    rows = ~np.isnan(r["want_inactive"])
    assert np.abs(inactive[rows] - r["want_inactive"][rows]).max(initial=0.0) <= TIGHT
    lens = np.diff(row_ptr)
    assert (inactive[lens == 0] == np.float32(1.0) / np.float32(r["O"])).all()
    # the walk over saturating pairs runs exactly where the output layer has pairs
    walk = net != "n256/256/nosat"  # (every other net of these cases has pairs in its output layer: HostModel.risky_pairs)
    if net in ("sat", "n256/256/nosat"):
        assert (api.HostModel(LC.model_path(net, fixtures)).risky_pairs(dnn.layerCount() - 1) > 0) == walk
    assert after[2] > before[2] and (after[1] > before[1]) == walk and (after[0] > before[0]) == (not walk)
    # the device form and the one-call form: the same bytes
    dp, di = device_form(dnn, x, row_ptr, nodes)
    assert same_bytes(dp, probs) and same_bytes(di, inactive)
    op, oi = dnn.calculateLazyLists(x, row_ptr, nodes)
    assert same_bytes(op, probs) and same_bytes(oi, inactive)
    # and the rows they stand for are the oracle's lazy rows
    full = F.lists_to_rows(row_ptr, nodes, probs, inactive, r["O"])
    assert np.abs(full - r["want_rows"]).max() <= TIGHT


@pytest.mark.parametrize("name", LC.RELATIVE)
def test_relative_bound_on_the_ladder_net(fixtures, name):
    """Prints softmax_ref.measure()-style figures (run with -s) for profiles/LABBOOK.md."""
    r = LC.reference(name, fixtures)
    dnn = model(LC.CASES[name][0], fixtures)
    probs, inactive = dnn.calculateLazyLists(r["x"], r["row_ptr"], r["nodes"])
    got = F.lists_to_rows(r["row_ptr"], r["nodes"], probs, inactive, r["O"])
    z = r["z"]
    p64 = SR.softmax64(z)
    assert not np.isnan(got).any() and (p64 >= SR.TINY).all()  # the second-class share is 0 (tests/test_lazy_lists_host.py)
    worst, worst_ratio, need_ce = 0.0, 0.0, 0.0
    for f in range(got.shape[0]):
        listed = r["masks"][f] != 0
        b = LC.relative_bound(z[f], listed, p64[f])
        rel = np.abs(got[f].astype(np.float64) / p64[f] - 1.0)
        worst, worst_ratio = max(worst, float(rel.max() / SR.U)), max(worst_ratio, float((rel / b).max()))
        A0 = np.where(listed, SR.L_ERR * np.abs(z[f].astype(np.float64)), 0.0)
        b0 = SR.U * (A0 + float((p64[f] * A0).sum()) + LC.depth(int(listed.sum())) + 2)
        slope = SR.U * (listed + float(p64[f][listed].sum()))  # the bound is linear in c_e
        with np.errstate(divide="ignore", invalid="ignore"):
            need_ce = max(need_ce, float(np.where(slope > 0, (rel - b0) / slope, -np.inf).max()))
        assert (rel <= b).all(), f"{name} row {f}: worst rel / bound {float((rel / b).max()):.3f}"
    print(f"\n[lists-range] {name}: worst_rel_u {worst:.2f}  worst_rel_over_bound {worst_ratio:.3f}  min_c_e {max(0.0, need_ce):.2f}", flush=True)


def test_tail_rows_that_overflow_equal_the_oracle(fixtures):
    name = "tail.ovf.n33"
    r = LC.reference(name, fixtures)
    dnn = model("tail/ovf", fixtures)
    probs, inactive = dnn.calculateLazyLists(r["x"], r["row_ptr"], r["nodes"])
    got = F.lists_to_rows(r["row_ptr"], r["nodes"], probs, inactive, r["O"])
    want = r["want_rows"]
    hot = np.isnan(want).any(1)
    assert hot[::2].all() and not hot[1::2].any()
    assert np.array_equal(got[hot], want[hot], equal_nan=True)  # four NaN, every other entry 0, inactive 0
    assert (np.isnan(got[hot]).sum(1) == 4).all() and (inactive[hot] == 0).all()
    rest = ~hot
    assert np.isfinite(got[rest]).all() and np.abs(got[rest] - want[rest]).max() <= TIGHT
    p64 = SR.softmax64(r["z"][rest])
    for g, zz, pp, mm in zip(got[rest], r["z"][rest], p64, r["masks"][rest]):
        rel = np.abs(g.astype(np.float64) / pp - 1.0)
        assert (pp >= SR.TINY).all() and (rel <= LC.relative_bound(zz, mm != 0, pp)).all()


def test_determinism_and_position(fixtures):
    """The same call twice: identical bytes.  A (frame, list) scored alone (count = 1, first = its row) and inside the
    700-row call: identical bytes -- also from another context whose rows start elsewhere."""
    r = LC.reference("mid.n700.s40", fixtures)
    dnn = model("mid", fixtures)
    x, row_ptr, nodes = r["x"], r["row_ptr"], r["nodes"]
    ctx = dnn.getNewLazyContext(700)
    ctx.calculateUntilOutput(x)
    p1, i1 = ctx.calculateForOutputNodesLists(row_ptr, nodes)
    p2, i2 = ctx.calculateForOutputNodesLists(row_ptr, nodes)
    assert same_bytes(p1, p2) and same_bytes(i1, i2)
    for f in (0, 1, 2, 3, 64, 333, 699):
        b, e = int(row_ptr[f]), int(row_ptr[f + 1])
        pa, ia = ctx.calculateForOutputNodesLists(np.array([0, e - b], np.int32), nodes[b:e], first=f)
        assert same_bytes(pa, p1[b:e]) and same_bytes(ia, i1[f:f + 1]), f
    # a block of rows at first > 0
    b, e = int(row_ptr[100]), int(row_ptr[164])
    pb, ib = ctx.calculateForOutputNodesLists(row_ptr[100:165] - row_ptr[100], nodes[b:e], first=100)
    assert same_bytes(pb, p1[b:e]) and same_bytes(ib, i1[100:164])
    ctx.delete()
    # frame 333 alone in a context of its own
    one = dnn.getNewLazyContext(1)
    one.calculateUntilOutput(x[333:334])
    b, e = int(row_ptr[333]), int(row_ptr[334])
    pc, ic = one.calculateForOutputNodesLists(np.array([0, e - b], np.int32), nodes[b:e])
    one.delete()
    assert same_bytes(pc, p1[b:e]) and same_bytes(ic, i1[333:334])


def test_list_calls_launch_nothing_of_the_masked_path(fixtures):
    r = LC.reference("mid.n100.s5", fixtures)
    dnn = model("mid", fixtures)
    ctx = dnn.getNewLazyContext(100)
    ctx.calculateUntilOutput(r["x"])
    before = api.lists_launches()
    api.launch_reset()
    api.launch_record(True)
    try:
        ctx.calculateForOutputNodesLists(r["row_ptr"], r["nodes"])
        names = api.launch_counts()
    finally:
        api.launch_record(False)
        ctx.delete()
    assert not [k for k in names if k.startswith(("gemm.out", "small.out", "ppo.out", "norm."))], names
    after = api.lists_launches()
    assert sum(after[:2]) == sum(before[:2]) + 1 and after[2] == before[2] + 1


def test_device_lists_with_a_node_past_the_layer(fixtures):
    """The device form does not validate: node O (inside the 1024 padded weight rows: a broken guard would read zeros, never
    fault) gives NaN for that row's entries and its inactive value; every other row keeps its bytes."""
    r = LC.reference("mid.n100.s40", fixtures)
    dnn = model("mid", fixtures)
    x, row_ptr, nodes = r["x"], r["row_ptr"], r["nodes"]
    good_p, good_i = device_form(dnn, x, row_ptr, nodes)
    f = 37
    b, e = int(row_ptr[f]), int(row_ptr[f + 1])
    bad = nodes.copy()
    bad[b + (e - b) // 2] = 1000
    p, i = device_form(dnn, x, row_ptr, bad)
    assert np.isnan(p[b:e]).all() and np.isnan(i[f])
    keep = np.ones(nodes.size, bool)
    keep[b:e] = False
    assert same_bytes(p[keep], good_p[keep]) and same_bytes(np.delete(i, f), np.delete(good_i, f))


def test_one_call_lists_from_many_threads(fixtures):
    """8 threads, own utterances and lists, pooled contexts (as test_one_call_lazy_from_many_threads)."""
    from oracle.oracle import Oracle

    dnn = model("mid", fixtures)
    orc = Oracle(fixtures["mid"])
    work = []
    for t in range(8):
        n = 50 + 13 * t
        x = F.synth_features(n, 432, seed=200 + t)
        m = F.generate_masks(n, 1000, 0.05 if t % 2 else 0.4, 0.03, seed=t)
        rp, nd = F.masks_to_lists(m)
        work.append((x, rp, nd, orc.lazy(x, m)))
    bad = []

    def run(t):
        x, rp, nd, want = work[t]
        for _ in range(10):
            p, i = dnn.calculateLazyLists(x, rp, nd)
            if not np.abs(F.lists_to_rows(rp, nd, p, i, 1000) - want).max() <= TIGHT:
                bad.append(t)

    th = [threading.Thread(target=run, args=(t,)) for t in range(8)]
    for h in th:
        h.start()
    for h in th:
        h.join()
    assert not bad


def test_errors(fixtures):
    r = LC.reference("mid.n8.s5", fixtures)
    dnn = model("mid", fixtures)
    x, row_ptr, nodes = r["x"], r["row_ptr"], r["nodes"]
    ctx = dnn.getNewLazyContext(8)
    with pytest.raises(api.FdnnError) as e:
        ctx.calculateForOutputNodesLists(row_ptr, nodes)  # before the hidden layers
    assert e.value.code == api.FDNN_E_STATE
    ctx.calculateUntilOutput(x)
    with pytest.raises(api.FdnnError) as e:
        ctx.calculateForOutputNodesLists(row_ptr, nodes, first=1)  # first + count > n
    assert e.value.code == api.FDNN_E_ARG
    desc = nodes.copy()
    b = int(row_ptr[5])
    desc[b], desc[b + 1] = nodes[b + 1], nodes[b]
    with pytest.raises(api.FdnnError) as e:
        ctx.calculateForOutputNodesLists(row_ptr, desc)
    assert e.value.code == api.FDNN_E_ARG and "row 5" in str(e.value)
    ctx.delete()
    p, i = np.empty(nodes.size, np.float32), np.empty(8, np.float32)
    rc = api.lib().fdnn_calculate_lazy_lists(dnn.nativeDnnHandle, x.ctypes.data_as(api._c_f32p), 8, 428, row_ptr.ctypes.data_as(api._c_i32p),
                                             nodes.ctypes.data_as(api._c_i32p), p.ctypes.data_as(api._c_f32p), i.ctypes.data_as(api._c_f32p))
    assert rc == api.FDNN_E_ARG  # a wrong dim in the one-call form
