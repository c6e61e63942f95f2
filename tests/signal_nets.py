"""Small nets that keep their signal, and the conditions each must meet before a GPU comparison on it means anything.
Plain helper module: numpy, formats and limit_nets only, no GPU, no fixture.

At synth_net's default scales (w0_std 0.02, w_std 0.05) a net narrower than ~512 forgets its input: over 200 frames the
median node of the last hidden layer moves by 0 bytes up to width 128, by 1 byte at 192 .. 272, by 3 at 512 ("small
nets that keep their signal").  Every frame then has nearly the same hidden row, and a kernel that read a neighbouring frame's
row, or a row of another frame tile, is judged on differences of 5e-5 in a probability.  The grid below states hotter scales per
width, at the K values that leave a wave's slice of the lazy-entry tile (fdnn_set_tile.hpp: 8 waves x 256 bytes of K) partly
filled -- one 16-byte chunk short (240, 2032), one chunk into the next wave (272), half the waves dead (1024) -- and output
widths 1, 3, 4 and 31 .. 2048 behind them.

  GRID    name -> (topology, frames, w0_std, w_std); net seed 11, features synth_features(n, in, seed=12, pad_from=None)
  MODES   gauss (saturating pairs: the walk instances run), nosat (none: the walk-free instances)
  CASES   (name, mode) of every net the tests use; NOSAT_LEFT_OUT says which widths have no walk-free variant and why

tests/test_signal_nets_host.py asserts the conditions below on the CPU oracle, case by case, so that
tests/test_gpu_signal_nets.py cannot pass on a net without signal."""
import os

import numpy as np

import limit_nets as LN

NET_SEED, FEATURE_SEED = 11, 12
MIN_RANGE = 48        # median over the nodes of (max - min) over the frames, last hidden layer, in bytes
MIN_VALUES = 200      # distinct byte values in the last hidden layer
ROLL_BAR = 2e-6       # a probability "moves" when it changes by more than the project's soft-max bar
MIN_ROLL_SHARE = 0.20 # share of the probabilities that move when every frame takes its neighbour's hidden row
TOPK_GAP = 8e-6       # a row's k-th and (k+1)-th probabilities are "apart": four times the bar (2e-6 either side, twice over)
MIN_TOPK_ROWS = 0.95  # share of the rows a top-k comparison against the oracle keeps


def _topo(d, h, o):
    return [d, h, h, h, o]


GRID = {
    "k16":   (_topo(4, 16, 3), 33, 0.3, 1.0),
    "k16b":  (_topo(4, 16, 3), 97, 0.3, 1.0),           # k16 over 97 frames: enough bytes for a walk-free variant (NOSAT_SCALE)
    "k48":   (_topo(12, 48, 31), 65, 0.3, 1.0),
    "k240":  (_topo(44, 240, 33), 129, 0.1, 0.3),      # 44, 132, 432 inputs: 11-frame splices of raw widths 4, 12, 39
    "k256":  (_topo(432, 256, 64), 97, 0.1, 0.3),
    "k272":  (_topo(132, 272, 257), 321, 0.1, 0.3),
    "k512":  (_topo(432, 512, 1001), 700, 0.05, 0.2),
    "k1024": (_topo(64, 1024, 2048), 641, 0.05, 0.2),  # 64 .. 496 inputs from 640 frames: the int8 layer-0 screening
    "k2032": (_topo(496, 2032, 65), 65, 0.02, 0.1),
    "k2048": (_topo(432, 2048, 251), 161, 0.02, 0.1),
    "o4":    (_topo(8, 96, 4), 63, 0.3, 0.6),
    "o1":    (_topo(40, 64, 1), 31, 0.3, 1.0),
}
MODES = ("gauss", "nosat")
RAW_DIM = {"k240": 4, "k272": 12, "k256": 39}  # the cases whose input is an 11-frame splice (the last padded from 429 to 432)

# synth_net's nosat mode clips the body at 3.2 sigma and plants one weight at 6.4 sigma, so that the body quantizes to
# |w_q| <= 64 -- as long as 6.4 sigma stays below the quantizer's absolute cut-off of 3.0, i.e. w_std <= 0.468.  At w_std 1.0
# (widths 16, 48, 64) outlier and body are clamped alike and the "nosat" net saturates as the gauss one does (oracle: 9, 249
# and 425 events).  The walk-free variants of those widths therefore take a scale of their own, found on the oracle: zero
# events, no risky pair in any layer, and the signal condition met.
NOSAT_SCALE = {"k48": (0.5, 0.4), "o1": (0.3, 0.4), "k16b": (3.0, 0.46)}   # oracle: median range 79.5 / 86.5 / 66.5 bytes, 250 / 252 / 210 values, 0 events
# Width 16 over 33 frames has no such scale: with w_std <= 0.468 the last hidden layer shows at most 182 distinct byte values
# for w0_std in 0.5 .. 5.0 (16 nodes x 33 frames = 528 bytes in all); above it pairs are risky again.  k16b is the same
# topology over 97 frames, where w0_std 3.0, w_std 0.46 reaches 210 values: K = 16 has its walk-free variant there.
NOSAT_LEFT_OUT = {"k16": "no scale with w_std <= 0.468 (6.4 sigma inside the quantizer's cut-off) reaches 200 distinct byte values at width 16 over 33 frames; k16b (97 frames) has the walk-free variant"}


def cases():
    return tuple((name, mode) for name in GRID for mode in MODES if not (mode == "nosat" and name in NOSAT_LEFT_OUT))


def case_id(name, mode):
    return f"{name}.{mode}"


def recipe(name, mode="gauss"):
    """-> (topology, frames, synth_net keywords)"""
    topo, n, w0, w = GRID[name]
    if mode == "nosat" and name in NOSAT_SCALE:
        w0, w = NOSAT_SCALE[name]
    return topo, n, dict(seed=NET_SEED, mode=mode, w0_std=w0, w_std=w)


def net(name, mode="gauss"):
    topo, _, kw = recipe(name, mode)
    return LN._F().synth_net(topo, **kw)


def path(name, mode="gauss", directory=None):
    """The case's net as a .bin in `directory` (TMPDIR by default), written unless it is there."""
    d = directory or os.environ.get("TMPDIR", "/tmp")
    topo, _, kw = recipe(name, mode)
    tag = f"signal_{name}_{mode}_{kw['w0_std']}_{kw['w_std']}".replace(".", "p")
    return LN.cached(d, tag, topo, lambda: net(name, mode))


def features(name, n=None):
    topo, frames, _ = recipe(name)
    return LN._F().synth_features(frames if n is None else n, topo[0], seed=FEATURE_SEED, pad_from=None)


# ------------------------------------------------------------------------------------------------------------- conditions
def signal_ok(u8_last):
    """(every row distinct, >= MIN_VALUES byte values, median node range >= MIN_RANGE) of one hidden layer's bytes [n][H]
    -> (ok, (distinct rows, median range, distinct values))"""
    frames, med, values = LN.signal_stats(u8_last)
    return bool(frames == u8_last.shape[0] and values >= MIN_VALUES and med >= MIN_RANGE), (frames, med, values)


def assert_keeps_signal(u8_last, what):
    ok, (frames, med, values) = signal_ok(u8_last)
    n = u8_last.shape[0]
    assert frames == n, f"{what}: only {frames} of {n} frames are distinct at the last hidden layer"
    assert values >= MIN_VALUES, f"{what}: only {values} distinct byte values at the last hidden layer"
    assert med >= MIN_RANGE, f"{what}: median per-node range {med} < {MIN_RANGE} at the last hidden layer"
    return frames, med, values


def roll_share(orc, u8_last, probs):
    """Share of the probabilities that move by more than ROLL_BAR when every frame is scored on its neighbour's hidden row."""
    rolled = orc.output_mt(np.roll(u8_last, 1, axis=0))
    return float((np.abs(rolled.astype(np.float64) - probs.astype(np.float64)) > ROLL_BAR).mean())


def topk_rows(probs, k):
    """bool [n]: the rows whose k-th and (k+1)-th largest probabilities are more than TOPK_GAP apart, so that the set of the k
    best nodes is the same for any result within 2e-6 of these rows twice over.  k >= O: every row (the set is all nodes)."""
    p = np.asarray(probs, dtype=np.float64)
    if k >= p.shape[1]:
        return np.ones(p.shape[0], bool)
    s = -np.sort(-p, axis=1)
    return (s[:, k - 1] - s[:, k]) > TOPK_GAP


def topk_ks(O):
    """The k of the top-k condition: 1 and min(5, O - 1) (none where the row has one node)."""
    return tuple(sorted({k for k in (1, min(5, O - 1)) if 1 <= k < O}))


def figures(orc, x):
    """Everything the conditions read, from the oracle alone -> dict(probs, taps, signal (ok, stats), roll, events, nan,
    topk {k: share of rows kept})"""
    probs, t = LN.taps_mt(orc, x)
    last = t["u8_acts"][-1]
    return dict(probs=probs, taps=t, signal=signal_ok(last), roll=roll_share(orc, last, probs), events=int(t["sat_events"]),
                nan=int(np.isnan(probs).sum()), topk={k: float(topk_rows(probs, k).mean()) for k in topk_ks(probs.shape[1])})


def arg_max_runs(probs):
    """Number of runs of the rows' arg-max: what the alignment transcripts are built from."""
    best = np.asarray(probs).argmax(axis=1)
    return int(1 + (best[1:] != best[:-1]).sum())
