"""A switched net whose pmaddubsw saturation events (dnn.cc:337-340) are known before anything runs, and a numpy replay
of the pair saturation.  Plain helper module: numpy only, no GPU, no fixture.

Why: the library reproduces the reference's int16 saturation of every adjacent pair a[2j] w[2j] + a[2j+1] w[2j+1] with a
sparse correction -- a screen per listed pair (one frame per lane, a ballot), the exact correction only when some lane
fires -- and seven kernels walk it, each on a schedule of its own over one shared arithmetic (fdnn_pair.hpp, checked on
the host by tests/host/pair_check.cpp).  The Gaussian fixtures either never fire it or fire the same few
entries on every frame; the hot nets fire in almost every frame.  Here every listed entry fires on exactly the frames the
caller switches it on in, and on no other.

The recipe (switch_net):
  * input columns 400 .. 400 + S - 1 are SWITCHES: shift 0, scale 1, value 0 or 1; the other columns carry synth_features;
  * every switch owns G = 16 RELAY nodes in every hidden layer, as 8 adjacent pairs (2k, 2k + 1) at pair positions chosen
    over the whole K (relay_pairs).  Layer-0 relay rows are zero but for weight 20 on their switch and bias -10: 255 when
    on, 0 when off.  Relay rows of the int8 hidden layers carry 0.25 on the 16 relay inputs of their switch and bias -2:
    0.25 quantises to 64, 255 * 128 = 32 640 cannot saturate, the relays stay at 225 / 215 (on) and 30 / 50 (off);
  * the body of every int8 layer is the synthetic Gaussian clipped to +-0.24 (|w_q| <= 61: no pair of it is listed), the
    layer multiplier is round(127 / 0.5) = 254;
  * a PROBE on node m at relay pair k is w[m, 2k] = s 0.5, w[m, 2k + 1] = s 0.48 (127 and 122): 249 * 215 > 32 767 when the
    pair's switch is on, 249 * 50 < 32 767 when it is off.  The probes are the layer's listed entries, all of them.

So with a switch on in one frame of a batch, every entry on that switch's pairs has an event on exactly one frame.
"""
from dataclasses import dataclass, field

import numpy as np

S = 8            # switches
G = 16           # relay nodes per switch and hidden layer (8 adjacent pairs)
SWITCH_COL = 400  # first switch column of the 432 inputs (400 .. 431 are kept free of features)
EVENT = np.dtype([("frame", np.int32), ("node", np.int32), ("pair", np.int32), ("sign", np.int8), ("excess", np.int32)])


@dataclass
class Plan:
    topology: list
    relay_pairs: np.ndarray           # [S][G / 2] pair index k (columns 2k, 2k + 1) of every switch's relays, the same in every hidden layer
    switch_of_pair: dict              # pair index -> switch
    probes: list = field(default_factory=list)  # per int8 layer (1 ..): int32 [P][4] rows (node, pair, sign, switch), by node then pair
    empty_groups: list = field(default_factory=list)  # per int8 layer: the 64-node groups left without entries on purpose

    def entries(self, layer):
        """(node, pair, sign, switch) of int8 layer `layer` (1 = the first int8 hidden layer)."""
        return self.probes[layer - 1]

    def planted(self, layer, switches_on):
        """The events of a batch: switches_on bool [n][S] -> sorted (frame, node, pair, sign) rows."""
        pr = self.entries(layer)
        out = []
        for f, s in zip(*np.nonzero(switches_on)):
            sel = pr[pr[:, 3] == s]
            out.append(np.column_stack([np.full(len(sel), f, np.int32), sel[:, :3]]))
        ev = np.concatenate(out) if out else np.zeros((0, 4), np.int32)
        return ev[np.lexsort((ev[:, 2], ev[:, 1], ev[:, 0]))]


def _relay_pairs(K, rng):
    """S * G / 2 = 64 pair positions over the K columns.  Fixed ones, as byte offsets: 0, the last pair of a 16-byte chunk
    (14), the first of the next (16), the last pair of a 64- and of a 128-byte k-step (62, 126), one pair in every 16-byte
    chunk index of a 128-byte step, the first pair of the last 128- and 64-byte step and the layer's last pair; the rest drawn."""
    fixed = [0, 14, 16, 62, 126, K - 128, K - 64, K - 50, K - 2]
    steps = K // 128
    fixed += [128 * ((c * 5 + 1) % steps) + 16 * c + 2 * (c % 8) for c in range(8)]
    fixed = list(dict.fromkeys(b // 2 for b in fixed))
    rest = np.setdiff1d(np.arange(K // 2), fixed)
    pairs = np.array(fixed + list(rng.choice(rest, S * G // 2 - len(fixed), replace=False)), dtype=np.int32)
    # bytes 0, 14, 16 share a 64-byte step: on three different switches, so that one node can carry two entries of one step
    order = np.concatenate([pairs[:3], rng.permutation(pairs[3:])])
    return order.reshape(G // 2, S).T.copy()  # [S][G / 2]: consecutive positions go to different switches


def switch_net(topology, seed=1, body_std=0.05, empty=None):
    """-> (FloatNet, Plan) for topology = [432, H, H, ..., W]: layer 0 in fp32, then int8 hidden layers and the int8 output layer.
    `empty`: per int8 layer the 64-node groups to leave without probes (default: group 1 of every layer, and of an output
    layer of more than 16 groups every group but the first three, one in the middle and the last two)."""
    from fast_dnn_amd import formats as F

    topology = [int(t) for t in topology]
    D, H, W = topology[0], topology[1], topology[-1]
    assert D >= SWITCH_COL + S and all(h == H for h in topology[1:-1]) and H % 128 == 0 and H >= 2 * S * G
    rng = np.random.default_rng(seed)
    net = F.synth_net(topology, seed=seed, w_std=body_std)
    rp = _relay_pairs(H, rng)
    sw_of = {int(k): s for s in range(S) for k in rp[s]}
    relay_cols = {s: np.sort(np.concatenate([2 * rp[s], 2 * rp[s] + 1])) for s in range(S)}
    relay_switch = np.full(H, -1, np.int32)  # hidden node -> the switch it relays, or -1
    for s in range(S):
        relay_switch[relay_cols[s]] = s
    net.shift[SWITCH_COL:] = 0.0
    net.scale[SWITCH_COL:] = 1.0
    L0 = net.layers[0]
    L0.weights[:, SWITCH_COL:] = 0.0  # the body does not see the switches
    for s in range(S):
        L0.weights[relay_cols[s], :] = 0.0
        L0.weights[relay_cols[s], SWITCH_COL + s] = 20.0
        L0.bias[relay_cols[s]] = -10.0
    plan = Plan(topology, rp, sw_of)
    n_q = len(topology) - 2
    all_pairs = rp.T.ravel()  # consecutive pairs: different switches
    for li in range(1, n_q + 1):
        L = net.layers[li]
        out_layer = li == n_q
        N = L.weights.shape[0]
        np.clip(L.weights, -0.24, 0.24, out=L.weights)
        if not out_layer:
            for s in range(S):
                L.weights[relay_cols[s], :] = 0.0
                L.weights[np.ix_(relay_cols[s], relay_cols[s])] = 0.25
                L.bias[relay_cols[s]] = -2.0
        groups = -(-N // 64)
        if empty is not None:
            skip = set(empty[li - 1])
        elif groups > 16 and out_layer:
            skip = set(range(groups)) - {0, 1 + li % 2, 2 + li % 2, groups // 2, groups - 2, groups - 1}
        else:
            skip = {1 + (li - 1) % 2}
        plan.empty_groups.append(sorted(skip))
        rows = []
        cursor = int(rng.integers(0, len(all_pairs)))
        for m in range(N):
            if m // 64 in skip:
                continue
            own = -1 if out_layer else int(relay_switch[m])
            while sw_of[int(all_pairs[cursor % len(all_pairs)])] == own:  # a probe never sits on a relay row of its own switch
                cursor += 1
            k = int(all_pairs[cursor % len(all_pairs)])
            cursor += 1
            rows.append((m, k, 1 if rng.random() < 0.5 else -1, sw_of[k]))
            # every 16th node of a group carries a second entry in the same 64-byte step: bytes 14 and 16 (or 0), other switches
            if m % 16 == 5 and own not in (sw_of[0], sw_of[7], sw_of[8]):
                first = {0: (7, 8), 7: (8, 0), 8: (0, 7)}.get(k, (7, 8))
                rows = [r for r in rows if r[0] != m]
                rows += [(m, first[0], 1, sw_of[first[0]]), (m, first[1], -1, sw_of[first[1]])]
        pr = np.array(sorted(set(rows)), dtype=np.int32)
        for m, k, sg, _ in pr:
            L.weights[m, 2 * k] = np.float32(0.5 * sg)
            L.weights[m, 2 * k + 1] = np.float32(0.48 * sg)
        plan.probes.append(pr)
    return net, plan


# kind -> (topology, std of the body of the int8 layers: 0.05 as the 256-wide fixtures, 0.02 as the K = 2048 hot tests)
NETS = {"k256.w256": ([432, 256, 256, 256, 256], 0.05), "k256.w252": ([432, 256, 256, 256, 252], 0.05),
        "k256.w251": ([432, 256, 256, 256, 251], 0.05), "k2048": ([432, 2048, 2048, 2048, 8000], 0.02)}
TDIV_BIAS = 1.5e7  # |lin| * 200 > 2e9: the layer fails the bounded-|lin| clause of the division check (fdnn_model.cpp: lin_bounded)


def true_divide_net(width=252):
    """The 256-wide switched net with one bias of 1.5e7 per int8 layer, on a node of the layer's empty group that relays no
    switch: the layer then takes the true-divide instances, listed pairs and all.  That node is 255 in every frame (its
    pairs with the body's |w_q| <= 61 stay below 32 767); the output row it sits in has no finite soft-max."""
    net, plan = switch_net([432, 256, 256, 256, int(width)], seed=11 + int(width) % 7, body_std=0.05)
    relay = {int(c) for k in plan.relay_pairs.ravel() for c in (2 * k, 2 * k + 1)}
    for li in range(1, len(net.layers)):
        g = plan.empty_groups[li - 1][0]
        node = next(m for m in range(64 * g, 64 * g + 64) if m not in relay)
        net.layers[li].bias[node] = np.float32(TDIV_BIAS)
    return net, plan


def model_file(directory, kind):
    """The net of `kind` ("tdiv.w252": true_divide_net) as a .bin in `directory`, written unless it is there -> (path, Plan)."""
    import os

    from fast_dnn_amd import formats as F

    if kind.startswith("tdiv.w"):
        net, plan = true_divide_net(int(kind[6:]))
    else:
        topo, std = NETS[kind]
        net, plan = switch_net(topo, seed=11 + topo[-1] % 7, body_std=std)
    p = os.path.join(directory, f"sat_switch_{kind}.bin")
    if not (os.path.exists(p) and os.path.getsize(p) == F.model_bin_size(plan.topology)):
        tmp = f"{p}.tmp{os.getpid()}"
        F.write_model_bin(tmp, net)
        os.replace(tmp, p)
    return p, plan


def features(n, switches_on, seed):
    """synth_features with columns 400 .. 431 cleared and the switches set: switches_on bool [n][S]."""
    from fast_dnn_amd import formats as F

    x = F.synth_features(n, 432, seed=seed)
    x[:, SWITCH_COL:] = 0.0
    x[:, SWITCH_COL:SWITCH_COL + S] = np.asarray(switches_on, dtype=np.float32)
    return x


def lone_switches(n, frames):
    """Switch s on in frame frames[s] only."""
    assert len(frames) == S and len(set(frames)) == S and all(0 <= f < n for f in frames), (n, frames)
    on = np.zeros((n, S), bool)
    on[np.asarray(frames), np.arange(S)] = True
    return on


def crowded_switches(n, seed):
    """One random switch on in half of the frames: the regime in which the screen's ballot is true for many lanes."""
    rng = np.random.default_rng(seed)
    on = np.zeros((n, S), bool)
    f = np.flatnonzero(rng.random(n) < 0.5)
    on[f, rng.integers(0, S, f.size)] = True
    return on


def lone_frames(n, T, Wf, rows=None, seed=0):
    """The S frames of a batch of n that carry one switch each: the in-tile rows 0, 31, 32, Wf - 1, Wf, T - 32, T - 1 (those
    below T), dealt over the first, a middle and the last (partial) tile, and the batch's last frame n - 1; where the tile
    has fewer distinct rows than switches the same rows of further tiles, then frames drawn by `seed`."""
    rows = sorted({r for r in ((0, 31, 32, Wf - 1, Wf, T - 32, T - 1) if rows is None else rows) if 0 <= r < T})
    tiles = -(-n // T)
    order = list(dict.fromkeys([0, tiles // 2, tiles - 1, tiles // 3, 1] if tiles > 1 else [0]))
    frames = [n - 1]

    def place(i, r, laps):
        for lap in laps:
            f = order[(i + lap) % len(order)] * T + r
            if f < n and f not in frames and len(frames) < S:
                frames.append(f)
                return

    for i, r in enumerate(rows):          # every row once, in the first tile of its turn that holds it
        place(i, r, range(len(order)))
    for lap in range(1, len(order)):      # then the same rows in further tiles
        for i, r in enumerate(rows):
            place(i, r, [lap])
    rng = np.random.default_rng(seed)
    while len(frames) < S:
        f = int(rng.integers(0, n))
        if f not in frames:
            frames.append(f)
    return frames[1:] + frames[:1]  # the last switch sits on n - 1


def pair_events(wq, acts):
    """pmaddubsw + pmaddwd + the int32 adds of quantizedNodeSum (dnn.cc:322-349), replayed: wq int8 [N][K], acts u8 [n][K] ->
    (events, acc).  events: EVENT records (frame, node, pair, sign, excess) of every pair whose sum leaves int16, sorted by
    frame, node, pair; excess = |p - sat16(p)|.  acc: int64 [n][N], the sum of the saturated pair sums.

    Only pairs with 255 (w0+ + w1+) > 32 767 or 255 (w0- + w1-) < -32 768 are examined pair by pair: for every other pair
    -32 768 <= 255 (w0- + w1-) <= p <= 255 (w0+ + w1+) <= 32 767 whatever the activations.  The unsaturated sums go through
    a float64 product, which is exact: |sum| <= K * 255 * 128 < 2^53."""
    wq = np.asarray(wq)
    acts = np.asarray(acts)
    assert wq.dtype == np.int8 and acts.dtype == np.uint8 and wq.shape[1] == acts.shape[1] and wq.shape[1] % 2 == 0
    w = wq.astype(np.int64)
    w0, w1 = w[:, 0::2], w[:, 1::2]
    can = (255 * (np.maximum(w0, 0) + np.maximum(w1, 0)) > 32767) | (255 * (np.minimum(w0, 0) + np.minimum(w1, 0)) < -32768)
    node, pair = np.nonzero(can)
    acc = np.rint(acts.astype(np.float64) @ wq.astype(np.float64).T).astype(np.int64)
    a = acts.astype(np.int64)
    p = a[:, 2 * pair] * w0[node, pair][None, :] + a[:, 2 * pair + 1] * w1[node, pair][None, :]
    d = np.clip(p, -32768, 32767) - p
    f, e = np.nonzero(d)
    np.add.at(acc, (f, node[e]), d[f, e])
    ev = np.zeros(f.size, dtype=EVENT)
    ev["frame"], ev["node"], ev["pair"] = f, node[e], pair[e]
    ev["sign"] = np.sign(p[f, e])
    ev["excess"] = np.abs(d[f, e])
    return np.sort(ev, order=["frame", "node", "pair"]), acc


def event_keys(ev):
    """EVENT records -> int32 [E][4] rows (frame, node, pair, sign), as Plan.planted returns them."""
    return np.column_stack([ev["frame"], ev["node"], ev["pair"], ev["sign"].astype(np.int32)]).astype(np.int32).reshape(-1, 4)
