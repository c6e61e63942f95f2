"""The switched nets of tests/sat_switch.py on the CPU oracle: the events are the planted ones and no others, they cover the
positions the GPU walks can get wrong, and dropping any one of them changes a byte.  No GPU.

Both sizes: 256-wide (the per-layer tiles, the small-batch kernels, the set / list kernels) and K = 2048 (the chained and the
role-split kernels)."""
import numpy as np
import pytest

import sat_switch as SS
from oracle.oracle import Oracle


@pytest.fixture(scope="module", params=list(SS.NETS))
def scored(request, tmp_models):
    """Every switch on in two frames of 48, no two switches in one frame; the oracle's taps and the numpy replay per int8 layer."""
    path, plan = SS.model_file(tmp_models, request.param)
    n = 48
    on = np.zeros((n, SS.S), bool)
    for s in range(SS.S):
        on[3 * s + 1, s] = on[24 + 3 * s + 2, s] = True
    x = SS.features(n, on, seed=77)
    orc = Oracle(path)
    _, wt = orc.calculate(x, taps=True)
    n_q = orc.n_layers - 1
    layers = []
    for li in range(1, n_q + 1):
        wq = orc.layer_wq(li)
        ev, acc = SS.pair_events(wq, wt["u8_acts"][li - 1])
        layers.append(dict(li=li, wq=wq, ev=ev, acc=acc, out=li == n_q, want=wt["acc_out"] if li == n_q else wt["acc_hid"][li - 1],
                           bias=orc.layer_bias(li), mult=orc.layer_mult(li), risky=orc.risky_pairs(li)))
    yield dict(kind=request.param, plan=plan, on=on, wt=wt, layers=layers, K=plan.topology[1])
    orc.close()


def test_the_listed_entries_are_the_probes(scored):
    for L in scored["layers"]:
        pr = scored["plan"].entries(L["li"])
        assert L["risky"] == len(pr)
        w = L["wq"].astype(np.int32)
        assert (np.abs(w[pr[:, 0], 2 * pr[:, 1]]) == 127).all() and (w[pr[:, 0], 2 * pr[:, 1] + 1] == 122 * pr[:, 2]).all()
        assert L["mult"] == 254.0


def test_events_are_the_planted_set_and_the_oracle_agrees_with_the_replay(scored):
    plan, on = scored["plan"], scored["on"]
    hidden_events = 0
    for L in scored["layers"]:
        planted = plan.planted(L["li"], on)
        assert len(planted) == 2 * len(plan.entries(L["li"]))
        assert np.array_equal(SS.event_keys(L["ev"]), planted), f"layer {L['li']}: the replay's events are not the planted set"
        assert np.array_equal(L["want"].astype(np.int64), L["acc"]), f"layer {L['li']}: the oracle's accumulators differ from the replay"
        # the oracle's own events: where its sums leave the exact ones, and by how much
        exact = np.rint(scored["wt"]["u8_acts"][L["li"] - 1].astype(np.float64) @ L["wq"].astype(np.float64).T).astype(np.int64)
        delta = np.zeros_like(exact)
        np.add.at(delta, (L["ev"]["frame"], L["ev"]["node"]), -L["ev"]["sign"].astype(np.int64) * L["ev"]["excess"])
        assert np.array_equal(L["want"] - exact, delta)
        assert set(np.flatnonzero(on.any(1))) == set(L["ev"]["frame"])  # 16 of the 48 frames carry events
        assert L["ev"]["excess"].min() > 10000
        if not L["out"]:
            hidden_events += len(L["ev"])
    assert scored["wt"]["sat_events"] == hidden_events


def test_residues_and_signs(scored):
    for L in scored["layers"]:
        pr = scored["plan"].entries(L["li"])
        N = L["wq"].shape[0]
        groups = sorted(set(pr[:, 0] // 64))
        assert len(groups) >= 3
        for g in groups:
            real = min(64, N - 64 * g)  # (a partial last group has no nodes beyond the layer's last)
            sel = pr[pr[:, 0] // 64 == g]
            assert set(sel[:, 0] % 64) == set(range(real)), (L["li"], g)
            assert {-1, 1} <= set(sel[:, 2]), (L["li"], g)
        ev = L["ev"]
        assert (ev["sign"] > 0).any() and (ev["sign"] < 0).any()
        assert set(ev["node"]) == set(pr[:, 0])


@pytest.mark.parametrize("BK", [128, 64])
def test_pair_positions_inside_a_k_step(scored, BK):
    K = scored["K"]
    for L in scored["layers"]:
        byte = 2 * L["ev"]["pair"].astype(np.int64)
        inside = set(byte % BK)
        assert {0, 14, 16, BK - 2} <= inside, (L["li"], BK)
        assert set((byte % BK) // 16) == set(range(BK // 16))
        steps = set(byte // BK)
        assert 0 in steps and K // BK - 1 in steps


def test_list_structure(scored):
    plan = scored["plan"]
    for L in scored["layers"]:
        pr = plan.entries(L["li"])
        N = L["wq"].shape[0]
        for BK in (128, 64):
            step = 2 * pr[:, 1] // BK
            grp = pr[:, 0] // 64
            _, cnt = np.unique(np.column_stack([grp, step]), axis=0, return_counts=True)
            assert cnt.max() >= 2                      # a group with two entries in one k-step
            _, cnt = np.unique(np.column_stack([pr[:, 0], step]), axis=0, return_counts=True)
            assert cnt.max() >= 2                      # two entries of one node in one k-step
        have = set(pr[:, 0] // 64)
        assert any(g not in have and g - 1 in have and any(h > g for h in have) for g in range(max(have)))  # an empty group between two others
        assert plan.empty_groups[L["li"] - 1] and not have & set(plan.empty_groups[L["li"] - 1])
        if L["out"]:
            assert N - 1 in set(pr[:, 0])              # the last real node (W = 251, 252: a partial 64-node group)


def test_every_event_is_visible(scored):
    """Dropping any single event's correction changes the node's output byte (hidden layers; in the output layer it changes the
    int32 accumulator by definition).  lin = f32(acc) / f32(mult * 255) + bias, the byte by QuantizedSigmoid::get."""
    for L in scored["layers"]:
        if L["out"]:
            assert (L["ev"]["excess"] != 0).all()
            continue
        coef = np.float32(np.float32(L["mult"]) * np.float32(255.0))
        ev = L["ev"]
        f, m = ev["frame"], ev["node"]
        acc = L["want"][f, m]
        dropped = acc + ev["sign"].astype(np.int64) * ev["excess"]
        lin = lambda a: (a.astype(np.float32) / coef).astype(np.float32) + L["bias"][m].astype(np.float32)
        with_fix = np.array([Oracle.sigmoid_q(float(v)) for v in lin(acc)])
        without = np.array([Oracle.sigmoid_q(float(v)) for v in lin(dropped)])
        assert np.array_equal(with_fix, scored["wt"]["u8_acts"][L["li"]][f, m])  # (the formula is the oracle's)
        invisible = int((with_fix == without).sum())
        assert invisible == 0, f"layer {L['li']}: {invisible} of {len(ev)} events would not show in the bytes"


def test_logits_stay_inside_exps_range(scored):
    z = scored["wt"]["logits"]
    assert z.min() > -87.0 and z.max() < 88.0


@pytest.mark.parametrize("n,T,Wf,rows", [(33, 32, 32, None), (545, 32, 32, None), (8257, 64, 64, None), (16513, 128, 64, None), (300, 128, 128, None),
                                         (33025, 256, 128, None), (65601, 320, 160, None), (641, 256, 128, None), (1281, 320, 160, None),
                                         (641, 320, 160, (0, 63, 64, 127, 128, 159, 160)), (961, 320, 160, (0, 63, 64, 127, 128, 159, 160))])
def test_lone_frames_sit_on_the_rows_of_the_case_table(n, T, Wf, rows):
    frames = SS.lone_frames(n, T, Wf, rows=rows, seed=n)
    assert len(set(frames)) == SS.S and all(0 <= f < n for f in frames) and frames[-1] == n - 1
    want = {r for r in (rows or (0, 31, 32, Wf - 1, Wf, T - 32, T - 1)) if r < T}
    assert want <= {f % T for f in frames}
    tiles = {f // T for f in frames}
    assert 0 in tiles and (n - 1) // T in tiles and (n <= 2 * T or len(tiles) >= 3)
    on = SS.lone_switches(n, frames)
    assert (on.sum(0) == 1).all() and on.sum() == SS.S
