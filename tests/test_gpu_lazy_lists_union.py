"""Lazy output by lists scored over per-frame-group node unions on the int8 MFMA (fdnn_model_set_lists_union;
fdnn_lists_union.hip).  The yardstick is exact: with the switch on, every list entry point returns the BYTES the same call
returns with the switch at 0 (the dot-product kernels of fdnn_lists.hip), the accumulators are the oracle's bit for bit,
and the probabilities stay within the project's 2e-6 of the oracle.  The fixtures and their references:
tests/lazy_lists_cases.py; the half that needs no GPU: tests/test_lazy_lists_union_host.py.

The models here are this module's own: the switch is a property of a model, and no other module's model ever sees it on."""
import numpy as np
import pytest

import dispatch_ledger as DL
import lazy_lists_cases as LC
from fast_dnn_amd import api, formats as F

pytestmark = pytest.mark.gpu
TIGHT = LC.TIGHT
SENTINEL = np.uint32(0xC0FFEE42)  # a bit pattern no result has (a negative float of magnitude ~8)

_MODELS = {}


@pytest.fixture(scope="module")
def fixtures(mid_model_path, sat_model_path, tiny_model_path, net_model_path):
    yield {"mid": mid_model_path, "sat": sat_model_path, "tiny": tiny_model_path, "full": net_model_path}
    LC.release()
    for d in _MODELS.values():
        d.delete()
    _MODELS.clear()


def model(net, fixtures):
    if net not in _MODELS:
        _MODELS[net] = api.QuantizedDnn.loadFromFile(LC.model_path(net, fixtures))
    _MODELS[net].setListsUnion(0)
    return _MODELS[net]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def off_and_on(dnn, g, call):
    """call() with the switch at 0 and at g -> (result off, result on, union counters' movement during the second call,
    list counters' movement during the second call); the switch is back at 0 afterwards."""
    try:
        dnn.setListsUnion(0)
        off = call()
        dnn.setListsUnion(g)
        ub, lb = api.lists_union_launches(), api.lists_launches()
        on = call()
        ua, la = api.lists_union_launches(), api.lists_launches()
    finally:
        dnn.setListsUnion(0)
    return off, on, tuple(a - b for a, b in zip(ua, ub)), tuple(a - b for a, b in zip(la, lb))


def device_call(dnn, x, row_ptr, nodes, first=0):
    """forward_hidden_device and the list call on ONE non-default stream, no synchronisation between them; d_probs (one word
    longer than nnz) and d_inactive pre-filled with SENTINEL -> (probs bits [nnz], inactive bits [count]) as uint32."""
    import torch

    n, count, nnz = x.shape[0], row_ptr.size - 1, nodes.size
    st = torch.cuda.Stream()
    dx = torch.from_numpy(x).cuda()
    drp = torch.from_numpy(row_ptr).cuda()
    dnd = torch.from_numpy(np.concatenate((nodes, np.zeros(1, np.int32)))).cuda()
    dp = torch.from_numpy(np.full(nnz + 1, SENTINEL, np.uint32).view(np.float32)).cuda()
    di = torch.from_numpy(np.full(count, SENTINEL, np.uint32).view(np.float32)).cuda()
    torch.cuda.synchronize()
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutputDevice(dx.data_ptr(), st.cuda_stream)
    ctx.calculateForOutputNodesListsDevice(drp.data_ptr(), dnd.data_ptr(), nnz, dp.data_ptr(), di.data_ptr(), first, count, st.cuda_stream)
    st.synchronize()
    probs, inactive = bits(dp.cpu().numpy()), bits(di.cpu().numpy())
    ctx.delete()
    assert probs[nnz] == SENTINEL  # nothing written past the entries
    return probs[:nnz].copy(), inactive


# ------------------------------------------------------------------------------------------- 1. byte identity and the oracle
@pytest.mark.parametrize("g", [1, 4])
@pytest.mark.parametrize("name", list(LC.CASES))
def test_union_path_returns_the_list_path_bytes_and_the_oracle_accumulators(fixtures, name, g):
    r = LC.reference(name, fixtures)
    net = LC.CASES[name][0]
    dnn = model(net, fixtures)
    x, row_ptr, nodes, n = r["x"], r["row_ptr"], r["nodes"], r["x"].shape[0]
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutput(x)
    try:
        (p0, i0), (p1, i1), moved, lmoved = off_and_on(dnn, g, lambda: ctx.calculateForOutputNodesLists(row_ptr, nodes))
        dnn.setListsUnion(g)
        acc = ctx.listsAccumulators(row_ptr, nodes)
    finally:
        dnn.setListsUnion(0)
        ctx.delete()
    diff_p = int((bits(p0) != bits(p1)).sum())
    diff_i = int((bits(i0) != bits(i1)).sum())
    want = r["want_probs"]
    finite = ~np.isnan(want)
    err = float(np.abs(p1[finite] - want[finite]).max(initial=0.0))
    print(f"\n[lists-union] {name} g{g}: nnz {nodes.size}  probs differing {diff_p}  inactive differing {diff_i}  "
          f"acc differing {int((acc != r['acc']).sum())}  max |p - oracle| {err:.3e}  counters {moved}", flush=True)
    assert diff_p == 0 and diff_i == 0
    assert np.array_equal(acc, r["acc"])
    assert np.array_equal(np.isnan(p1), ~finite) and err <= TIGHT
    rows = ~np.isnan(r["want_inactive"])
    assert np.abs(i1[rows] - r["want_inactive"][rows]).max(initial=0.0) <= TIGHT
    # which instance: the walk over saturating pairs runs exactly where the output layer has pairs
    walk = api.HostModel(LC.model_path(net, fixtures)).risky_pairs(dnn.layerCount() - 1) > 0
    assert walk == (net != "n256/256/nosat") or net in ("lad/256", "tail/ovf")  # sat.* walks, nosat.* does not
    assert moved == ((1, 0, 1, 0) if walk else (1, 1, 0, 0))
    assert lmoved == (0, 0, 1)
    if name == "mid.special.n4":
        lens = np.diff(row_ptr)
        assert lens.tolist() == [0, 1000, 1, 1] and nodes[1000] == 0 and nodes[1001] == 999
        assert bits(i1)[0] == bits(np.float32(1.0) / np.float32(1000.0))
    if name == "tail.ovf.n33":
        assert np.isnan(p1).sum() == 4 * 17


# ------------------------------------------------------------------------------------------- 2. group seams
def _seam_masks(n, what):
    m = F.generate_masks(n, 1000, 0.05, 0.03, seed=300 + n)
    if what == "hole":
        m[32:64] = 0  # rows 32 .. 63: a group (g = 1) whose union is empty
    if what == "empty":
        m[:] = 0
    return m


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("n,first,what", [(1, 0, ""), (31, 0, ""), (32, 0, ""), (33, 0, ""), (65, 0, ""),
                                          (1, 5, ""), (31, 5, ""), (32, 5, ""), (33, 5, ""), (65, 5, ""),
                                          (65, 0, "hole"), (70, 5, "hole"), (33, 0, "empty")])
def test_group_seams(fixtures, n, first, what, g):
    """Groups are counted from the call's first row: the same rows at first = 5 of a 100-frame context fall into the same
    groups.  A group whose rows are all empty has u_len 0 and no work item; a call without entries launches the finish only."""
    dnn = model("mid", fixtures)
    total = 100 if first else n
    x = F.synth_features(total, 432, seed=40 + n)
    row_ptr, nodes = F.masks_to_lists(_seam_masks(n, what))
    ctx = dnn.getNewLazyContext(total)
    ctx.calculateUntilOutput(x)
    try:
        (p0, i0), (p1, i1), moved, lmoved = off_and_on(dnn, g, lambda: ctx.calculateForOutputNodesLists(row_ptr, nodes, first=first))
    finally:
        ctx.delete()
    assert same_bytes(p0, p1) and same_bytes(i0, i1), (int((bits(p0) != bits(p1)).sum()), int((bits(i0) != bits(i1)).sum()))
    assert i1.size == n and not np.isnan(i1).any()
    if what == "empty":
        assert nodes.size == 0 and moved == (0, 0, 0, 0) and lmoved == (0, 0, 1)
        assert (bits(i1) == bits(np.float32(1.0) / np.float32(1000.0))).all()
    else:
        assert moved == (1, 0, 1, 0) and lmoved == (0, 0, 1)
    if what == "hole":
        assert (np.diff(row_ptr)[32:64] == 0).all() and (bits(i1[32:64]) == bits(np.float32(1.0) / np.float32(1000.0))).all()


# ------------------------------------------------------------------------------------------- 3. the union build alone
@pytest.mark.parametrize("case,g", [("mid.n100.s5", 1), ("mid.n100.s5", 2), ("wide33", 1), ("wide33", 8)])
def test_union_build_kernel_equals_the_host_restatement(fixtures, case, g):
    dnn = model("mid", fixtures)
    if case == "wide33":  # 33 rows of 40 %: two groups for g = 1, unions far longer than one 64-node chunk
        x = F.synth_features(33, 432, seed=33)
        row_ptr, nodes = F.masks_to_lists(F.generate_masks(33, 1000, 0.4, 0.03, seed=33))
    else:
        r = LC.reference(case, fixtures)
        x, row_ptr, nodes = r["x"], r["row_ptr"], r["nodes"]
    want = api.lists_union_ref(row_ptr, nodes, 1000, g)
    ctx = dnn.getNewLazyContext(x.shape[0])
    ctx.calculateUntilOutput(x)
    before = api.lists_union_launches()
    got = ctx.listsUnion(row_ptr, nodes, g)
    after = api.lists_union_launches()
    ctx.delete()
    assert tuple(a - b for a, b in zip(after, before)) == (1, 0, 0, 0)
    for k, what in enumerate(("u_len", "u_nodes", "pos")):
        assert np.array_equal(got[k], want[k]), what
    assert (want[2] >= 0).all() and want[0].size == -(-x.shape[0] // (32 * g))
    if case == "wide33":
        assert want[0].max() > 64


# ------------------------------------------------------------------------------------------- 4. the device form, unvalidated
def test_device_lists_with_nodes_outside_the_layer(fixtures):
    """-1, output_dim and 2^31 - 1 in three rows of one group and its neighbour: those rows are NaN throughout, inactive too,
    every other row keeps the clean call's bytes -- and nothing was used as an address (the sentinel past the entries holds)."""
    r = LC.reference("mid.n100.s40", fixtures)
    dnn = model("mid", fixtures)
    x, row_ptr, nodes = r["x"], r["row_ptr"], r["nodes"]
    bad = nodes.copy()
    hit = {7: -1, 37: 1000, 64: 2 ** 31 - 1}
    for f, v in hit.items():
        b, e = int(row_ptr[f]), int(row_ptr[f + 1])
        assert e - b >= 3
        bad[b + (e - b) // 2] = v
    for g in (1, 4):
        try:
            dnn.setListsUnion(g)
            clean_p, clean_i = device_call(dnn, x, row_ptr, nodes)
            p, i = device_call(dnn, x, row_ptr, bad)
            dnn.setListsUnion(0)
            old_p, old_i = device_call(dnn, x, row_ptr, bad)
        finally:
            dnn.setListsUnion(0)
        keep = np.ones(nodes.size, bool)
        for f in hit:
            b, e = int(row_ptr[f]), int(row_ptr[f + 1])
            keep[b:e] = False
            assert np.isnan(p[b:e].view(np.float32)).all() and np.isnan(i[f:f + 1].view(np.float32)).all(), (g, f)
        rows = np.array([f not in hit for f in range(100)])
        assert np.array_equal(p[keep], clean_p[keep]) and np.array_equal(i[rows], clean_i[rows]), g
        assert np.array_equal(p, old_p) and np.array_equal(i, old_i), g  # NaN payloads included
        assert not (p == SENTINEL).any() and not (i == SENTINEL).any()


def test_device_lists_with_a_duplicate_and_a_descending_row(fixtures):
    """Every entry is written exactly once whatever the order: no sentinel survives, and the bytes are the dot-product
    kernels' on the same lists."""
    r = LC.reference("mid.n100.s40", fixtures)
    dnn = model("mid", fixtures)
    x, row_ptr, nodes = r["x"], r["row_ptr"], r["nodes"]
    odd = nodes.copy()
    b, e = int(row_ptr[12]), int(row_ptr[13])
    odd[b + 1] = odd[b]  # a duplicate
    odd[b + 5] = odd[b]  # and once more, further on
    b, e = int(row_ptr[50]), int(row_ptr[51])
    odd[b:e] = odd[b:e][::-1].copy()  # a descending row
    old_p, old_i = device_call(dnn, x, row_ptr, odd)
    for g in (1, 4):
        try:
            dnn.setListsUnion(g)
            p, i = device_call(dnn, x, row_ptr, odd)
        finally:
            dnn.setListsUnion(0)
        assert not (p == SENTINEL).any() and not (i == SENTINEL).any(), g
        assert np.array_equal(p, old_p) and np.array_equal(i, old_i), g
    assert not (old_p == SENTINEL).any()


# ------------------------------------------------------------------------------------------- 5. which kernel ran
def test_switch_off_moves_no_union_counter_and_bad_values_are_refused(fixtures):
    r = LC.reference("mid.n100.s5", fixtures)
    dnn = model("mid", fixtures)
    ctx = dnn.getNewLazyContext(100)
    ctx.calculateUntilOutput(r["x"])
    ub, lb = api.lists_union_launches(), api.lists_launches()
    ctx.calculateForOutputNodesLists(r["row_ptr"], r["nodes"])
    ua, la = api.lists_union_launches(), api.lists_launches()
    assert ua == ub and tuple(a - b for a, b in zip(la, lb)) == (0, 1, 1)
    for badv in (9, -2, 100):
        with pytest.raises(api.FdnnError) as e:
            dnn.setListsUnion(badv)
        assert e.value.code == api.FDNN_E_ARG
    # -1: on, with the library's default group; the same bytes
    try:
        p0, i0 = ctx.calculateForOutputNodesLists(r["row_ptr"], r["nodes"])
        dnn.setListsUnion(-1)
        ub = api.lists_union_launches()
        p1, i1 = ctx.calculateForOutputNodesLists(r["row_ptr"], r["nodes"])
        ua = api.lists_union_launches()
    finally:
        dnn.setListsUnion(0)
        ctx.delete()
    assert tuple(a - b for a, b in zip(ua, ub)) == (1, 0, 1, 0) and same_bytes(p0, p1) and same_bytes(i0, i1)


def test_a_layer_the_tile_does_not_stage_goes_to_the_dot_product_kernels(fixtures):
    """dispatch_ledger's 'k2304' net: K = 2304 is more than the tile stages, so with the switch on the call is counted as a
    fallback ([3]) and served by the list kernels: the switch-at-0 bytes by construction."""
    dnn = model("k2304", fixtures)
    O = dnn.outputDimension()
    x = F.synth_features(33, 432, seed=23)
    row_ptr, nodes = F.masks_to_lists(F.generate_masks(33, O, 0.2, 0.03, seed=4))
    ctx = dnn.getNewLazyContext(33)
    ctx.calculateUntilOutput(x)
    try:
        (p0, i0), (p1, i1), moved, lmoved = off_and_on(dnn, 2, lambda: ctx.calculateForOutputNodesLists(row_ptr, nodes))
    finally:
        ctx.delete()
    assert moved == (0, 0, 0, 1) and sum(lmoved[:2]) == 1 and lmoved[2] == 1
    assert same_bytes(p0, p1) and same_bytes(i0, i1)


# ------------------------------------------------------------------------------------------- 6. one call and streams
def test_one_call_form_in_two_chunks(fixtures):
    """fdnn_calculate_lazy_lists at the smallest n that fdnn_debug_frame_chunks cuts in two: every chunk is a call of its
    own with its lists rebased, its groups counted from the chunk's first row."""
    lo, hi = 1, 1 << 17
    assert len(api.frame_chunks(lo)) == 1 and len(api.frame_chunks(hi)) >= 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if len(api.frame_chunks(mid)) >= 2:
            hi = mid
        else:
            lo = mid
    n = hi
    assert len(api.frame_chunks(n)) == 2 and len(api.frame_chunks(n - 1)) == 1
    dnn = model("mid", fixtures)
    x = F.synth_features(n, 432, seed=66)
    row_ptr, nodes = F.masks_to_lists(F.generate_masks(n, 1000, 0.02, 0.03, seed=67))
    (p0, i0), (p1, i1), moved, lmoved = off_and_on(dnn, 2, lambda: dnn.calculateLazyLists(x, row_ptr, nodes))
    print(f"\n[lists-union] one call, n {n}: chunks {api.frame_chunks(n)}  counters {moved}", flush=True)
    assert moved[0] == moved[2] and moved[0] >= 2 and moved[1] == 0 and moved[3] == 0 and lmoved == (0, 0, moved[0])
    assert same_bytes(p0, p1) and same_bytes(i0, i1)


def test_a_list_call_on_a_stream_context(fixtures):
    """fdnn_stream_push(out = NULL) leaves the pushed frames' hidden activations in the stream's context; a list call on it
    with the switch on returns the bytes of the same with it at 0."""
    dnn = model("mid", fixtures)
    raw = np.random.default_rng(9).standard_normal((70, 39)).astype(np.float32) * 3
    dnn.setSplice(list(range(-5, 6)), 39)
    st = None
    try:
        st = dnn.newStream(72)
        ctx = st.pushHidden(raw, end=True)
        k = ctx.inputVectorCount
        assert k == 70
        row_ptr, nodes = F.masks_to_lists(F.generate_masks(k, 1000, 0.05, 0.03, seed=70))
        (p0, i0), (p1, i1), moved, lmoved = off_and_on(dnn, 2, lambda: ctx.calculateForOutputNodesLists(row_ptr, nodes))
    finally:
        if st is not None:
            st.close()
        dnn.setSplice([], 0)
    assert moved == (1, 0, 1, 0) and lmoved == (0, 0, 1)
    assert same_bytes(p0, p1) and same_bytes(i0, i1) and not np.isnan(p1).any()
