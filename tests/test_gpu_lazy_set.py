"""Lazy output for a shared node set (fdnn_ctx_lazy_output_set / _device, fdnn_calculate_lazy_set; fdnn_set.hip) against the
oracle, with the MFMA kernel forced (fdnn_debug_set_kernel(1)): the int32 accumulators bit for bit, probabilities and
inactive values within 2e-6 of Oracle.lazy's rows, the bytes of fdnn_ctx_lazy_output_lists with the set repeated per row, the
same bytes from the host form, the device form, the one-call form, the fallback and from any row range -- and on the ladder
net within lazy_lists_cases.relative_bound of float64.  The fixtures and their references: tests/lazy_set_cases.py
(tests/test_lazy_set_host.py shows that the normative sum order itself meets these bars)."""
import threading

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


def has_pairs(net, fixtures):
    return api.HostModel(LC.model_path(net, fixtures)).risky_pairs(model(net, fixtures).layerCount() - 1) > 0


def same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def set_buffers(nodes, count):
    """Device buffers of one set call, a sentinel past count * len and past count: (nodes, probs, inactive)"""
    import torch

    dnd = torch.from_numpy(np.concatenate((nodes, np.zeros(1, np.int32)))).cuda()
    dp = torch.full((count * nodes.size + 1,), -7.0, dtype=torch.float32, device="cuda")
    di = torch.full((count + 1,), -7.0, dtype=torch.float32, device="cuda")
    return dnd, dp, di


def read_back(bufs, count, length):
    probs, inactive = bufs[1].cpu().numpy(), bufs[2].cpu().numpy()
    assert probs[count * length] == -7.0 and inactive[count] == -7.0  # nothing written past the results
    return probs[:count * length].reshape(count, length), inactive[:count]


def device_form(dnn, x, sets, first, count):
    """forward_hidden_device and one set call per entry of `sets` on ONE non-default stream, no synchronisation between
    them -> [(probs [count][len], inactive [count]) per set]"""
    import torch

    st = torch.cuda.Stream()
    dx = torch.from_numpy(x).cuda()
    bufs = [set_buffers(nd, count) for nd in sets]
    torch.cuda.synchronize()
    ctx = dnn.getNewLazyContext(x.shape[0])
    ctx.calculateUntilOutputDevice(dx.data_ptr(), st.cuda_stream)
    for nd, b in zip(sets, bufs):
        ctx.calculateForOutputNodeSetDevice(b[0].data_ptr(), nd.size, b[1].data_ptr(), b[2].data_ptr(), first, count, st.cuda_stream)
    st.synchronize()
    ctx.delete()
    return [read_back(b, count, nd.size) for nd, b in zip(sets, bufs)]


@pytest.mark.parametrize("name", [c for c in SC.CASES if c not in SC.RELATIVE + SC.TAIL + SC.FALLBACK_BY_SHAPE])
def test_set_against_the_oracle_through_every_entry_point(fixtures, name):
    case = SC.CASES[name]
    r = SC.reference(name, fixtures)
    dnn = model(case.net, fixtures)
    x, nodes, n, L, O = r["x"], r["nodes"], case.n, r["nodes"].size, case.O
    walk = has_pairs(case.net, fixtures)
    assert walk == (case.net != "n256/256/nosat")
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutput(x)
    for first, count in case.ranges:
        rows = slice(first, first + count)
        sb, lb = api.set_launches(), api.lists_launches()
        probs, inactive = ctx.calculateForOutputNodeSet(nodes, first, count)
        sa, la = api.set_launches(), api.lists_launches()
        # the MFMA kernel ran, with the pair walk exactly where the layer has pairs; of the list kernels only the finish pass
        if L:
            assert (sa[1] > sb[1]) == walk and (sa[0] > sb[0]) == (not walk) and sa[2] == sb[2]
        assert la[0] == lb[0] and la[1] == lb[1] and la[2] > lb[2]
        acc = ctx.setAccumulators(nodes, first, count)
        assert np.array_equal(acc, r["acc"][rows]), f"{name} {first}+{count}: {int((acc != r['acc'][rows]).sum())} accumulators differ from the oracle"
        print(f"\n[set] {name} rows {first}+{count}: max |p - oracle| {np.abs(probs - r['want_probs'][rows]).max(initial=0.0):.3e}", flush=True)
        assert probs.shape == (count, L) and np.abs(probs - r["want_probs"][rows]).max(initial=0.0) <= TIGHT
        want_i = r["want_inactive"][rows]
        known = ~np.isnan(want_i)
        assert np.abs(inactive[known] - want_i[known]).max(initial=0.0) <= TIGHT
        if L == 0:
            assert (inactive == np.float32(1.0) / np.float32(O)).all()
        # the bytes of the list path with the set repeated per row
        lp, li = ctx.calculateForOutputNodesLists(SC.uniform_row_ptr(count, L), np.tile(nodes, count), first=first)
        assert same_bytes(lp.reshape(count, L), probs) and same_bytes(li, inactive)
        # the fallback: the same bytes, no MFMA launch
        api.set_kernel(2)
        try:
            sb = api.set_launches()
            fp, fi = ctx.calculateForOutputNodeSet(nodes, first, count)
            sa = api.set_launches()
        finally:
            api.set_kernel(1)
        assert same_bytes(fp, probs) and same_bytes(fi, inactive)
        assert sa[:2] == sb[:2] and (sa[2] > sb[2]) == (L > 0)
        # the device form and the one-call form: the same bytes
        (dp, di), = device_form(dnn, x, [nodes], first, count)
        assert same_bytes(dp, probs) and same_bytes(di, inactive)
        op, oi = dnn.calculateLazySet(x[rows], nodes)
        assert same_bytes(op, probs) and same_bytes(oi, inactive)
        # and the rows they stand for are the oracle's lazy rows
        full = F.lists_to_rows(SC.uniform_row_ptr(count, L), np.tile(nodes, count), probs.ravel(), inactive, O)
        assert np.abs(full - r["want_rows"][rows]).max() <= TIGHT
    # a row's bytes do not depend on the range it was scored in: alone as [r, r + 1) against the widest range
    first, count = max(case.ranges, key=lambda fc: fc[1])
    probs, inactive = ctx.calculateForOutputNodeSet(nodes, first, count)
    for row in sorted({first, first + 1, first + count // 2, first + count - 1}):
        p1, i1 = ctx.calculateForOutputNodeSet(nodes, row, 1)
        assert same_bytes(p1, probs[row - first:row - first + 1]) and same_bytes(i1, inactive[row - first:row - first + 1]), row
    ctx.delete()


def test_one_call_form_in_two_chunks(fixtures):
    """fdnn_calculate_lazy_set at the smallest n that api.frame_chunks cuts in two, on the tiny net: every chunk scores the
    same set and its rows land at probs + off * len, its inactive values at off -- the bytes of the same rows as two calls."""
    n = 20480 + 1
    for chained in (True, False):
        assert len(api.frame_chunks(n, chained)) == 2 and len(api.frame_chunks(n - 1, chained)) == 1
    cut = api.frame_chunks(n, True)[1][0]
    dnn = api.QuantizedDnn.loadFromFile(fixtures["tiny"])
    nodes = np.arange(3, 100, 3, dtype=np.int32)  # 33 of the tiny net's 100 nodes
    x = F.synth_features(n, 432, seed=1310)
    probs, inactive = dnn.calculateLazySet(x, nodes)
    a, b = dnn.calculateLazySet(x[:cut], nodes), dnn.calculateLazySet(x[cut:], nodes)
    assert probs.shape == (n, nodes.size) and np.array_equal(probs.view(np.uint32), np.concatenate([a[0], b[0]]).view(np.uint32))
    assert np.array_equal(inactive.view(np.uint32), np.concatenate([a[1], b[1]]).view(np.uint32))
    dnn.delete()


def test_a_layer_the_kernel_does_not_stage_goes_to_the_list_kernels(fixtures):
    """K = 2304 is more than the kernel stages: under the default rule and with the MFMA kernel 'forced' the call is served by
    the list kernels, within the same bars."""
    name = SC.FALLBACK_BY_SHAPE[0]
    case = SC.CASES[name]
    r = SC.reference(name, fixtures)
    dnn = model(case.net, fixtures)
    ctx = dnn.getNewLazyContext(case.n)
    ctx.calculateUntilOutput(r["x"])
    results = []
    for mode in (0, 1):
        api.set_kernel(mode)
        sb = api.set_launches()
        results.append(ctx.calculateForOutputNodeSet(r["nodes"]))
        sa = api.set_launches()
        assert sa[:2] == sb[:2] and sa[2] == sb[2] + 1
    (probs, inactive), (p0, i0) = results[1], results[0]
    assert same_bytes(p0, probs) and same_bytes(i0, inactive)
    assert np.array_equal(ctx.setAccumulators(r["nodes"]), r["acc"])
    lp, li = ctx.calculateForOutputNodesLists(r["row_ptr"], r["list_nodes"])
    ctx.delete()
    assert same_bytes(lp.reshape(probs.shape), probs) and same_bytes(li, inactive)
    assert np.abs(probs - r["want_probs"]).max() <= TIGHT and np.abs(inactive - r["want_inactive"]).max() <= TIGHT


@pytest.mark.parametrize("name", SC.RELATIVE)
def test_relative_bound_on_the_ladder_net(fixtures, name):
    """Every element within lazy_lists_cases.relative_bound of float64 (DEPTH for the set's len); prints the figures (-s)."""
    r = SC.reference(name, fixtures)
    dnn = model(SC.CASES[name].net, fixtures)
    n, L = r["x"].shape[0], r["nodes"].size
    sb = api.set_launches()
    probs, inactive = dnn.calculateLazySet(r["x"], r["nodes"])
    sa = api.set_launches()
    assert sum(sa[:2]) > sum(sb[:2]) and sa[2] == sb[2]
    got = F.lists_to_rows(r["row_ptr"], r["list_nodes"], probs.ravel(), inactive, r["O"])
    z = r["z"]
    p64 = SR.softmax64(z)
    assert not np.isnan(got).any() and (p64 >= SR.TINY).all()
    worst, worst_ratio = 0.0, 0.0
    for f in range(n):
        listed = r["masks"][f] != 0
        b = LC.relative_bound(z[f], listed, p64[f])
        rel = np.abs(got[f].astype(np.float64) / p64[f] - 1.0)
        worst, worst_ratio = max(worst, float(rel.max() / SR.U)), max(worst_ratio, float((rel / b).max()))
        assert (rel <= b).all(), f"{name} row {f}: worst rel / bound {float((rel / b).max()):.3f}"
    print(f"\n[set-range] {name}: len {L}  worst_rel_u {worst:.2f}  worst_rel_over_bound {worst_ratio:.3f}", flush=True)


def test_a_set_with_the_overflowing_logits_equals_the_oracle(fixtures):
    dnn = model("tail/ovf", fixtures)
    r = SC.reference("tail.ovf.hot", fixtures)
    probs, inactive = dnn.calculateLazySet(r["x"], r["nodes"])
    got = F.lists_to_rows(r["row_ptr"], r["list_nodes"], probs.ravel(), inactive, r["O"])
    assert np.array_equal(got, r["want_rows"], equal_nan=True)  # four NaN, every other entry 0, inactive 0
    assert (np.isnan(got).sum(1) == 4).all() and (inactive == 0).all()
    r = SC.reference("tail.ovf.cold", fixtures)
    probs, inactive = dnn.calculateLazySet(r["x"], r["nodes"])
    got = F.lists_to_rows(r["row_ptr"], r["list_nodes"], probs.ravel(), inactive, r["O"])
    assert np.isfinite(got).all() and np.abs(got - r["want_rows"]).max() <= TIGHT


@pytest.mark.parametrize("bad", [1000, -1])
def test_device_set_with_a_node_outside_the_layer(fixtures, bad):
    """The device form does not validate: node O (inside the 1024 padded weight rows) or node -1 in the set is never used as
    an address (fdnn_set.hpp's guard, tests/host/set_check.cpp); its column's e is NaN, so every row's entries and inactive
    value are NaN -- and the next, valid call on the same context is correct."""
    r = SC.reference(f"mid.len{SC.NT + 1}", fixtures)
    dnn = model("mid", fixtures)
    x, nodes = r["x"], r["nodes"]
    wrong = nodes.copy()
    wrong[SC.NT // 2] = bad
    (p, i), (gp, gi) = device_form(dnn, x, [wrong, nodes], 0, 100)
    assert np.isnan(p).all() and np.isnan(i).all()
    assert np.abs(gp - r["want_probs"]).max() <= TIGHT and np.abs(gi - r["want_inactive"]).max() <= TIGHT


def test_two_threads_on_their_own_contexts(fixtures):
    r = SC.reference(f"mid.len{2 * SC.NT + 1}", fixtures)
    dnn = model("mid", fixtures)
    x, nodes = r["x"], r["nodes"]
    ctx = dnn.getNewLazyContext(100)
    ctx.calculateUntilOutput(x)
    want_p, want_i = ctx.calculateForOutputNodeSet(nodes)
    ctx.delete()
    bad = []

    def run(t):
        c = dnn.getNewLazyContext(100)
        for _ in range(5):
            c.calculateUntilOutput(x)
            p, i = c.calculateForOutputNodeSet(nodes)
            if not (same_bytes(p, want_p) and same_bytes(i, want_i)):
                bad.append(t)
        c.delete()

    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for h in th:
        h.start()
    for h in th:
        h.join()
    assert not bad


def test_errors(fixtures):
    r = SC.reference("mid.len1", fixtures)
    dnn = model("mid", fixtures)
    x = r["x"]
    ctx = dnn.getNewLazyContext(100)
    with pytest.raises(api.FdnnError) as e:
        ctx.calculateForOutputNodeSet([1, 2])  # before the hidden layers
    assert e.value.code == api.FDNN_E_STATE
    ctx.calculateUntilOutput(x)
    with pytest.raises(api.FdnnError) as e:
        ctx.calculateForOutputNodeSet([1, 2], first=1, count=100)  # first + count > n
    assert e.value.code == api.FDNN_E_ARG
    for wrong in ([2, 1], [1, 1], [-1, 3], [3, 1000]):
        with pytest.raises(api.FdnnError) as e:
            ctx.calculateForOutputNodeSet(wrong)
        assert e.value.code == api.FDNN_E_ARG
    ctx.delete()
    nd = np.array([1, 2], np.int32)
    p, i = np.empty((8, 2), np.float32), np.empty(8, np.float32)
    rc = api.lib().fdnn_calculate_lazy_set(dnn.nativeDnnHandle, x.ctypes.data_as(api._c_f32p), 8, 428, nd.ctypes.data_as(api._c_i32p), 2,
                                           p.ctypes.data_as(api._c_f32p), i.ctypes.data_as(api._c_f32p))
    assert rc == api.FDNN_E_ARG  # a wrong dim in the one-call form
