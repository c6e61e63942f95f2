"""Nets at the limits of what the loader accepts (read_raw_model, fdnn_model.cpp), and the condition each must meet before a
GPU comparison on it means anything.  Plain helper module: numpy and the CPU oracle only, no GPU, no fixture.

  deep_net         up to 29 int8 hidden layers that keep their signal: the default Gaussian net collapses with depth (at
                   layer 29 of [432] + [256] * 30 + [252] only 8 of 64 frames are distinct and a node moves by 0.05 of a byte
                   over the batch), so a kernel that read the wrong frame, tile or buffer would still match the oracle
  wide_out_net     an output layer of up to 2^19 nodes whose logits span exp's range with every probability a normal fp32
  extreme_acc_net  K = 4112: accumulators beyond 2^26 in magnitude whose quotients sit on ties of the sigmoid table
  d_net            input widths either side of the layer-0 rules' edges

tests/test_limit_nets_host.py asserts the conditions below on the CPU, so that tests/test_gpu_model_limits.py cannot pass
on a degenerate net."""
import os
import struct

import numpy as np

import softmax_ref as SR

MIN_RANGE = 64     # median over the nodes of (max - min) over the sampled frames, last hidden layer, in bytes
MIN_VALUES = 128   # distinct byte values in the last hidden layer of the sampled frames


def _F():
    from fast_dnn_amd import formats as F

    return F


def cached(directory, name, topology, make):
    """The net make() returns as `name`.bin in `directory`, written unless a file of the right size is there -> path."""
    F = _F()
    p = os.path.join(directory, name + ".bin")
    if not (os.path.exists(p) and os.path.getsize(p) == F.model_bin_size(topology)):
        tmp = f"{p}.tmp{os.getpid()}"
        F.write_model_bin(tmp, make())
        os.replace(tmp, p)
    return p


def taps_mt(orc, x):
    """Oracle.calculate(taps=True) over frame ranges in parallel (frames are independent) -> (probs, taps)."""
    from concurrent.futures import ThreadPoolExecutor

    ch = orc._chunks(len(x), orc.default_threads())
    with ThreadPoolExecutor(len(ch)) as ex:
        parts = list(ex.map(lambda r: orc.calculate(x[r[0]:r[1]], taps=True), ch))
    wt = {k: np.concatenate([t[k] for _, t in parts], axis=1 if k in ("u8_acts", "acc_hid") else 0) for k in ("u8_acts", "acc_hid", "acc_out", "logits")}
    wt["sat_events"] = sum(t["sat_events"] for _, t in parts)
    return np.concatenate([w for w, _ in parts]), wt


# ---------------------------------------------------------------------------------------------------------------- depth
# (int8 hidden layers, w_std) of every depth the tests use: both sides of the chained launch's 8 layers, two and three
# launches with and without a one-layer tail, the loader's limit; 0.5 once, so that the correction walk runs deep too
DEPTHS = ((2, 0.3), (7, 0.3), (8, 0.3), (9, 0.3), (16, 0.3), (17, 0.5), (29, 0.3))


def deep_topology(n_hidden, width=256, out=252):
    """n_hidden int8 hidden layers behind the fp32 layer 0: n_hidden + 2 affine layers (the loader takes 4 .. 31)."""
    return [432] + [int(width)] * (int(n_hidden) + 1) + [int(out)]


def deep_net(n_hidden, width=256, out=252, seed=7, w_std=0.3):
    """synth_net with hot int8 weights, every int8 HIDDEN layer's rows made zero-mean.

    The activations of a sigmoid layer share a positive mean (~128); through Gaussian rows that common mean, times the
    row's weight sum, drives every node of the next layer alike and the net forgets its input within a few layers.  With
    zero-mean rows only the differences between activations pass, and w_std = 0.3 keeps them large.

    Condition (assert_keeps_signal): at the LAST hidden layer of the sampled frames every frame is distinct, the median
    per-node range is >= 64 bytes and >= 128 distinct byte values occur.  w_std = 0.5 saturates harder (range 254) and fires
    ~20 times as many pair-saturation events: the correction walk then runs at every depth too."""
    net = _F().synth_net(deep_topology(n_hidden, width, out), seed=seed, w_std=w_std)
    for L in net.layers[1:-1]:
        L.weights -= L.weights.mean(axis=1, keepdims=True, dtype=np.float64).astype(np.float32)
    return net


def signal_stats(u8):
    """u8 [n][H], one hidden layer's bytes -> (distinct frames, median per-node range, distinct byte values)."""
    u8 = np.asarray(u8)
    rng = u8.max(axis=0).astype(np.int32) - u8.min(axis=0).astype(np.int32)
    return len(np.unique(u8, axis=0)), float(np.median(rng)), len(np.unique(u8))


def assert_keeps_signal(u8_last, what):
    n = u8_last.shape[0]
    frames, med, values = signal_stats(u8_last)
    assert frames == n, f"{what}: only {frames} of {n} sampled frames are distinct at the last hidden layer"
    assert med >= MIN_RANGE, f"{what}: median per-node range {med} < {MIN_RANGE} at the last hidden layer"
    assert values >= MIN_VALUES, f"{what}: only {values} distinct byte values at the last hidden layer"
    return frames, med, values


# --------------------------------------------------------------------------------------------------------- output width
def wide_out_topology(W, hidden=16):
    return [432, int(hidden), int(hidden), int(hidden), int(W)]


def wide_out_net(W, hidden=16):
    """A narrow net in front of W output nodes, output biases a shuffled ladder over [-40, 20] (tests/softmax_ref.py).
    Condition (test_limit_nets_host.py): no float64 probability of the sampled frames lies below 2^-126, so
    _softmax_rel_ok's `share == 0` holds and every entry is held to the relative bound."""
    net = _F().synth_net(wide_out_topology(W, hidden))
    net.layers[-1].bias = SR.ladder(int(W), -40.0, 20.0, seed=int(W))
    return net


def edge_nodes(W, count=80, seed=3):
    """A node set of `count` nodes with node 0, node W - 1 and both sides of every multiple of 65 536 below W."""
    must = {0, W - 1}
    for m in range(65536, W + 1, 65536):
        must.update(v for v in (m - 1, m) if 0 <= v < W)
    rng = np.random.default_rng(seed + W)
    while len(must) < count:
        must.add(int(rng.integers(0, W)))
    assert len(must) == count, (W, len(must))
    return np.array(sorted(must), dtype=np.int32)


# --------------------------------------------------------------------------------------------------------- hidden width
ACC_H = 4112          # x16, no multiple of 128, above 4096: (H / 2) * 32768 > 2^26
ACC_ROWS = 16         # planted rows of the second int8 hidden layer: 0 .. 7 positive, 8 .. 15 negative
ACC_TIES = (12.5, 37.5, 62.5, 87.5, 112.5, 137.5)   # see extreme_acc_net
ACC_OFFSETS = (0, 0, 1, 0, 0, -1, 0, 0)             # ulps of 100 lin off the tie, by planted row (mod 8)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def ulp_step(v, k):
    """fp32 v moved by k ulps away from (k > 0) / towards (k < 0) zero."""
    i = f32(v).view(np.int32)
    return np.int32(i + k).view(np.float32)


def plain_wide_hidden_net(H=ACC_H, seed=81):
    """The ordinary shapes at K = 4112: a Gaussian net, nothing planted."""
    return _F().synth_net([432, H, H, H, 252], seed=seed)


def extreme_acc_skeleton(H=ACC_H, seed=81):
    """extreme_acc_net before its 16 biases are solved (those rows' biases are 0) -> (net, c)."""
    net = plain_wide_hidden_net(H, seed)
    L1, L2 = net.layers[1], net.layers[2]
    # first int8 hidden layer: bias +9 and weights a tenth of the usual (|acc / coef| stays below 1): 100 lin >= 640 in
    # every node and every frame, the table's last entry: every activation is 255
    L1.weights *= np.float32(0.1)
    L1.bias[:] = 9.0
    c = np.float32(np.abs(L2.weights).max())  # the layer's abs-max: +-c quantises to +-127 and leaves the multiplier as it is
    for r in range(ACC_ROWS):
        L2.weights[r, :] = c if r < ACC_ROWS // 2 else -c
        L2.weights[r, :2 * (r % (ACC_ROWS // 2))] = 0.0  # row r: r mod 8 pairs zeroed -> 16 different accumulators
        L2.bias[r] = 0.0
    return net, c


def hidden_lin(acc, coef, bias):
    """The reference's pre-activation of an int8 layer: f32(f32(acc) / coef) + bias (dnn.cc:311)."""
    return (f32(acc.astype(np.float32)) / np.float32(coef)).astype(np.float32) + f32(bias)


def extreme_acc_net(net, acc_rows, coef, lut_at):
    """extreme_acc_skeleton's `net` ([432, H, H, H, 252], H = 4112) with its 16 biases solved, in place: the second int8
    hidden layer then has 16 rows with accumulators beyond 2^26 whose quotients sit on table ties.

    The first int8 hidden layer outputs 255 everywhere (extreme_acc_skeleton).  Rows 0 .. 7 of the second are +c, rows 8 .. 15
    -c (w_q = +-127): every pair is 255 * 254 = 64 770 before saturation, +32 767 / -32 768 after it, so a row of P pairs
    accumulates 32 767 P or -32 768 P.  Row r has r mod 8 of its 2056 pairs zeroed: 2049 .. 2056 pairs, |acc| from 67 139 583
    to 67 371 008, all beyond 2^26 = 67 108 864 = 2048 * 32 768 -- the range the load-time division sweep used to stop at.
    (More than 7 zeroed pairs would fall back inside it: 2048 * 32 767 < 2^26.)

    acc_rows: the ORACLE's accumulators of those rows (they do not depend on the biases of their own layer); coef: the
    layer's divisor f32(mult * 255); lut_at(lin) -> byte (Oracle.sigmoid_q).  The 16 biases are walked by ulps, as
    tests/test_gpu_l0_edge.py::edge_net does, until fl(100 * fl(fl(acc / coef) + b)) is a table tie h + 0.5 or 1 ulp off one.
    The quotient is ~ +-540, so lin = q + b moves on the grid 2^-14 of q's ulp, and 100 lin reaches h + 0.5 only where
    (2 h + 1) / 200 is a multiple of 2^-14: h + 0.5 in 12.5, 37.5, ... (odd multiples of 0.125 in lin).  Those are ACC_TIES,
    signed by row; the rows asked for a tie (12 of 16) land on it exactly, the others on the nearest grid point.  One ulp
    of the quotient is one grid step, 0.006 in 100 lin: from a tie it changes the rounded index, and the ties are taken where
    the table's two entries differ, so a quotient wrong by one ulp changes the byte.

    -> (net, info): info["hit"] rows that landed exactly, info["lin"], info["want_t"], info["sensitive_in"] /
    info["sensitive_out"] rows whose byte changes when the quotient moves by one ulp towards / away from zero."""
    acc_rows = np.asarray(acc_rows).astype(np.int64)
    assert acc_rows.shape == (ACC_ROWS,)
    q = (acc_rows.astype(np.float32) / np.float32(coef)).astype(np.float32)
    hundred = np.float32(100.0)
    ties = [t for t in ACC_TIES if lut_at(float(np.float32(t - 0.25) / hundred)) != lut_at(float(np.float32(t + 0.25) / hundred))]
    assert len(ties) >= 3, ties
    bias = np.zeros(ACC_ROWS, np.float32)
    lin = np.zeros(ACC_ROWS, np.float32)
    want = np.zeros(ACC_ROWS, np.float32)
    hit = np.zeros(ACC_ROWS, bool)
    for r in range(ACC_ROWS):
        sign = 1.0 if (r // 2) % 2 == 0 else -1.0
        target_t = np.float32(sign * ties[r % len(ties)])
        want_t = ulp_step(target_t, ACC_OFFSETS[r % len(ACC_OFFSETS)])
        b0 = np.float32(np.float64(want_t) / 100.0 - np.float64(q[r]))
        best = None
        for k in range(-64, 65):
            b = ulp_step(b0, k)
            tt = np.float32(np.float32(q[r] + b) * hundred)
            d = abs(int(tt.view(np.int32)) - int(want_t.view(np.int32)))
            if best is None or d < best[0]:
                best = (d, b)
            if d == 0:
                break
        bias[r], hit[r], want[r] = best[1], best[0] == 0, want_t
        lin[r] = np.float32(q[r] + bias[r])
    net.layers[2].bias[:ACC_ROWS] = bias
    # rounding is half away from zero: from a tie one direction of the quotient's error changes the index, the other does not
    moved = {k: np.array([lut_at(float(np.float32(ulp_step(q[r], k) + bias[r]))) != lut_at(float(lin[r])) for r in range(ACC_ROWS)]) for k in (-1, 1)}
    return net, dict(hit=hit, lin=lin, want_t=want, q=q, bias=bias, sensitive_in=moved[-1], sensitive_out=moved[1])


def planted_acc(H=ACC_H):
    """What the reference accumulates on the planted rows when every input is 255: 32 767 per pair of a +127 row, -32 768
    per pair of a -127 row (pmaddubsw's int16 saturation, dnn.cc:337-340)."""
    pairs = H // 2 - np.arange(ACC_ROWS) % (ACC_ROWS // 2)
    return np.where(np.arange(ACC_ROWS) < ACC_ROWS // 2, 32767 * pairs, -32768 * pairs).astype(np.int64)


def extreme_acc_file(directory, H=ACC_H, seed=81):
    """extreme_acc_net as a .bin in `directory`, written unless it is there (142 MB) -> (path, info).  The biases are solved
    from planted_acc() and the oracle's own quantizer; info["acc"] is that prediction, and every user asserts that the
    oracle's acc_hid on the planted rows IS it (assert_planted) -- so they are solved from the oracle's accumulators."""
    from oracle.oracle import Oracle

    net, _ = extreme_acc_skeleton(H, seed)  # (built once; the biases are solved into it)
    _, mult = Oracle.quantize(net.layers[2].weights)
    coef = np.float32(np.float32(mult) * np.float32(255.0))
    acc = planted_acc(H)
    net, info = extreme_acc_net(net, acc, coef, Oracle.sigmoid_q)
    info.update(acc=acc, coef=coef)
    return cached(directory, f"limit_extreme_acc_{H}", [432, H, H, H, 252], lambda: net), info


def assert_planted(info, wt, orc):
    """The oracle's taps `wt` of any batch on extreme_acc_file's net: the planted rows' accumulators are the predicted ones,
    beyond 2^26, in every frame; the layer's divisor is the one the biases were solved for."""
    got = wt["acc_hid"][1][:, :ACC_ROWS].astype(np.int64)
    assert (wt["u8_acts"][1] == 255).all(), "the first int8 hidden layer is not 255 everywhere"
    assert np.array_equal(got, np.broadcast_to(info["acc"], got.shape)), "the oracle's accumulators on the planted rows are not the predicted ones"
    assert (np.abs(got) > (1 << 26)).all()
    assert np.float32(np.float32(orc.layer_mult(2)) * np.float32(255.0)) == info["coef"]


# ---------------------------------------------------------------------------------------------------------- input width
# 496 / 500: l0_split_ok; 596 / 600: the small kernel's LDS (l0_small_geom: 161 856 / 163 904 bytes against 163 840; 608, 612
# and 616 lie above that edge); 4096 / 4100: can_screen (fdnn_select.hpp)
D_WIDTHS = (496, 500, 596, 600, 608, 612, 616, 4096, 4100, 8192)


def d_topology(D):
    return [int(D), 64, 64, 64, 100]


def d_net(D):
    return _F().synth_net(d_topology(D), seed=500 + int(D) % 97, w0_std=0.01)


# --------------------------------------------------------------------------------------------------------- loader limits
def write_header_only(path, topology, full_layers):
    """A .bin whose first `full_layers` layers are complete (zero weights) and whose next layer is its 8-byte header only:
    what the loader refuses from a layer's header it refuses before it asks for that layer's weights."""
    with open(path, "wb") as f:
        f.write(struct.pack(">i", len(topology) - 1))
        for i in range(1, full_layers + 2):
            f.write(struct.pack(">ii", topology[i - 1], topology[i]))
            if i <= full_layers:
                f.write(bytes(4 * (topology[i - 1] * topology[i] + topology[i])))
    return path
