"""The half net's sums on a FIXED-POINT operand grid, where the float64 sum IS the fp32 result.  numpy only, no GPU.

csrc/fdnn_half.hpp's contract holds a sum to float64 under a bound, because the order of the additions inside one MFMA is the
hardware's.  On this grid the order cannot matter:

    x = i / 8 (i in +-{1 .. 8}),  w = j / 16 (j in +-{1 .. 16}),  b = m / 128 (|m| <= 256)

are exact halves, every product x w = i j / 128 and every partial sum of products and bias is an integer multiple of 2^-7, and
while 128 (sum |x w| + |b|) stays below 2^24 every such partial sum is an fp32 value.  So every addition of every order is
exact and z EQUALS the float64 sum bit for bit: no tolerance.  `premise` returns that magnitude; the tests keep it below 2^22,
two bits under the significand for an adder that aligns the terms of an instruction before it adds them.  Every term is
non-zero, so a lost, repeated or skipped k-step, a stale ring slot, a neighbouring row of W or a neighbouring bias changes the
exact value and cannot pass, at any K (tests/test_half_exact_host.py holds each of these; tests/test_gpu_half_exact.py the
kernels).
"""
import numpy as np

from fast_dnn_amd import formats as F

GRID = 128  # every term, bias and sum is a multiple of 1 / GRID
LIMIT = 2 ** 22  # the tests' cap on `premise`: two bits under the fp32 significand


def _x(rng, n, K):
    return (rng.integers(1, 9, (n, K)) * rng.choice([-1, 1], (n, K)) / 8.0).astype(np.float32)


def _w(rng, rows, K):
    return (rng.integers(1, 17, (rows, K)) * rng.choice([-1, 1], (rows, K)) / 16.0).astype(np.float32)


def _b(rows, seed):
    """m / 128, |m| <= 256; 37 is no multiple of 513, so neighbouring rows differ by at least 1 / 128."""
    return ((((np.arange(rows) + seed) * 37) % 513 - 256) / 128.0).astype(np.float32)


def grid_case(n, rows, K, seed):
    """x [n][K], w [rows][K], b [rows] on the grid of the module docstring; every term non-zero."""
    rng = np.random.default_rng(seed)
    return _x(rng, n, K), _w(rng, rows, K), _b(rows, seed)


def premise(x, w, b):
    """128 (sum_k |x_k w_k| + |b|) at its maximum over the outputs: the largest magnitude, in grid units, that any partial sum
    of any order of additions can reach."""
    S = np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(w, np.float64)).T + np.abs(np.asarray(b, np.float64))[None, :]
    return float(GRID * S.max())


def want64(x, w, b):
    return np.asarray(x, np.float64) @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)[None, :]


def want(x, w, b):
    """The float64 sums cast to fp32 (the cast is exact under the premise: test_half_exact_host holds it)."""
    return want64(x, w, b).astype(np.float32)


def net(D, H, O, seed):
    """FloatNet [D, H, H, H, O], shift 0 and scale 1, every layer on the grid: layer 0 a sigmoid layer with K = D (D H floats:
    the K sweep of the sigmoid forms is cheap), the output layer an exp layer with K = H."""
    rng = np.random.default_rng(seed)
    dims = (D, H, H, H, O)
    layers = [F.FloatLayerSpec(_w(rng, o, i), _b(o, seed + j)) for j, (i, o) in enumerate(zip(dims, dims[1:]))]
    return F.FloatNet(layers, np.zeros(D, np.float32), np.ones(D, np.float32))


def rows_for(net_, j, n, seed):
    """n grid rows for layer j of such a net (the debug call takes the caller's rows for any layer)."""
    return _x(np.random.default_rng(seed), n, net_.layers[j].in_dim)


# ------------------------------------------------------------------------------------------------------------ the case tables
# The kernel settings of a layer call (setSmall, setMid) and its frame counts.  small: FT = 1 .. 4 frame tiles of 32; mid: two
# and three frame tiles of 64, the last one a single frame; tiled: the second frame tile of 256 holds one frame.
RUNS = (("small", 128, 0, (31, 64, 65, 128)), ("mid", 0, 4096, (65, 129)), ("hgemm", 0, 0, (257,)))
N_ROWS = 257

# The sigmoid forms: K swept through layer 0 of net(D, 80, 64).  Every multiple of 32 up to 1280 (every K_pad residue of the
# 128-k and the 256-k stages after up to ten and five full ones), the bench width and the first K_pad past it, 4112 (K_pad
# 4128: 34 tiles of the small kernel's NT = FT = 1 stream, more than two 9-tile rings), and two D that are no multiples of
# 32: K_pad 1056 and 2048 with live -0 pad columns in W.
SIG_H, SIG_O = 80, 64
SIG_D = tuple(range(32, 1281, 32)) + (2048, 2080, 4112, 1044, 2044)

# The exp forms and the set kernel: K swept through H of net(20, H, 131).  288 is there for the mid kernel's two-step last
# stage after two full ones, which none of the others has in the exp form (96 + 128 i is six steps, 1088 four, 2048 eight).
EXP_D, EXP_O = 20, 131
EXP_H = (96, 224, 288, 352, 480, 608, 736, 864, 1072)
EXP_H_WIDE = 2048  # a test of its own: the longest
SET_LENS, SET_N = (1, 33, 131), (33, 65)
HIDDEN_N = {"small": 65, "mid": 129, "hgemm": 257}  # layers 1 and 2 (sigmoid, K = H, H rows: many node tiles): one n per kernel


def sig_case(D):
    """The net of one D of the sigmoid sweep and the rows of its layer 0."""
    nt = net(D, SIG_H, SIG_O, seed=D)
    return nt, rows_for(nt, 0, N_ROWS, seed=D + 1)


def exp_case(H):
    """The net of one H of the exp sweep and the rows of its layers 1, 2 and 3."""
    nt = net(EXP_D, H, EXP_O, seed=H)
    return nt, {j: rows_for(nt, j, N_ROWS, seed=H + j) for j in (1, 2, 3)}


def operand_cases():
    """Every (name, x, w, b) the GPU tests hold a kernel to."""
    for D in SIG_D:
        nt, x = sig_case(D)
        yield f"sigmoid D {D}", x, nt.layers[0].weights, nt.layers[0].bias
    for H in EXP_H + (EXP_H_WIDE,):
        nt, xs = exp_case(H)
        for j in (1, 2, 3):
            yield f"H {H} layer {j}", xs[j], nt.layers[j].weights, nt.layers[j].bias


def k_pad(K):
    return -(-K // 32) * 32


def rows_pad(rows):
    return -(-rows // 256) * 256


def layer_calls():
    """Every dense layer call of the GPU tests -> (form, kernel, K, rows, n): what the coverage checks count."""
    out = []
    for kernel, _, _, ns in RUNS:
        out += [("sigmoid", kernel, D, SIG_H, n) for D in SIG_D for n in ns]
        for H in EXP_H + (EXP_H_WIDE,):
            out += [("exp", kernel, H, EXP_O, n) for n in ns]
            out.append(("sigmoid", kernel, H, H, HIDDEN_N[kernel]))
    return out


# ------------------------------------------------------------------------------------------------------------ the plain forms
# calculate() returns probabilities only, so the non-tap forms need nets that keep signal through multi-stage K: Gaussian
# nets with w_std = 0.3 sqrt(48 / H) for every layer (the tiny net's 0.3 at H = 48, the pre-activation's spread kept).
PLAIN = {"k352": ([228, 352, 352, 352, 131], 31), "k608": ([1044, 608, 608, 608, 257], 32)}


def plain_net(name):
    topology, seed = PLAIN[name]
    std = 0.3 * np.sqrt(48.0 / topology[1])
    return F.synth_net(topology, seed=seed, w0_std=std, w_std=std)


def plain_features(name):
    return F.synth_features(N_ROWS, PLAIN[name][0][0], seed=4, pad_from=None)
