"""What tests/test_gpu_half_exact.py rests on, without a device (tests/half_exact.py): the fixed-point premise of every case,
that fp32 accumulation in any order then equals the float64 sum bit for bit, that every planted fault changes the value, that
the case tables reach every k-loop shape of the four kernels, and that the Gaussian nets of the plain forms keep signal."""
import os
import re

import numpy as np
import pytest

import float_ref as FR
import half_exact as HE
import half_ref as HR
from conftest import ROOT
from fast_dnn_amd import api

CSRC = os.path.join(ROOT, "fast-dnn_amd", "csrc")


def _const(file, pattern):
    m = re.search(pattern, open(os.path.join(CSRC, file)).read())
    assert m, (file, pattern)
    return int(m.group(1))


# The kernels' k-loop constants, restated here and read back from their sources so that a change there fails this file:
TILED_K = 32    # fdnn_float.hpp:23 kKStep (fdnn_half.hpp:55): one LDS stage of hgemm_kernel, two MFMAs deep
MID_K = 128     # fdnn_half_mid.hip:78 kStageK
MID_RING = 2    # fdnn_half_mid.hip:83 kRingStages
SMALL_K = 256   # fdnn_half_small.hip:63 kStageK
SMALL_RING = 9  # fdnn_half_small.hip:67 FDNN_HSMALL_RING_TILES -> kRingTiles
SET_K = 256     # fdnn_half_set.hpp:42 kBlockK


def test_the_restated_constants_are_the_kernels():
    assert _const("fdnn_float.hpp", r"constexpr int kKStep = (\d+);") == TILED_K
    assert _const("fdnn_half_mid.hip", r"constexpr int kStageK = (\d+);") == MID_K
    assert _const("fdnn_half_mid.hip", r"constexpr int kRingStages = (\d+);") == MID_RING
    assert _const("fdnn_half_small.hip", r"constexpr int kStageK = (\d+);") == SMALL_K
    assert _const("fdnn_half_small.hip", r"#define FDNN_HSMALL_RING_TILES (\d+)") == SMALL_RING
    assert _const("fdnn_half_set.hpp", r"constexpr int kBlockK = (\d+);") == SET_K


@pytest.fixture(scope="module")
def cases():
    return list(HE.operand_cases())


def _sample(x, w, b, seed):
    """Six frames and eight rows of a case, the first and the last of each among them."""
    rng = np.random.default_rng(seed)
    f = np.unique(np.concatenate(([0, x.shape[0] - 1], rng.integers(0, x.shape[0], 4))))
    r = np.unique(np.concatenate(([0, w.shape[0] - 1], rng.integers(0, w.shape[0], 6))))
    return f, r


def test_premise_and_operands(cases):
    """Every case: the grid, no zero term, neighbouring biases apart, the premise below 2^22, the float64 sums fp32 values."""
    assert len(cases) == len(HE.SIG_D) + 3 * (len(HE.EXP_H) + 1)
    worst = 0.0
    for name, x, w, b in cases:
        assert x.dtype == w.dtype == b.dtype == np.float32, name
        for a, scale, top in ((x, 8, 8), (w, 16, 16), (b, 128, 256)):
            g = a.astype(np.float64) * scale
            assert np.array_equal(g, np.rint(g)) and np.abs(g).max() <= top, name
            assert np.array_equal(a, HR.halves(a)), name  # exact in fp16: the loader and the debug call round nothing away
        assert (x != 0).all() and (w != 0).all() and (np.abs(np.diff(b)) >= 1.0 / 128).all(), name
        p = HE.premise(x, w, b)
        worst = max(worst, p)
        assert p < HE.LIMIT, (name, p)
        z64 = HE.want64(x, w, b)
        assert np.array_equal(HE.want(x, w, b).astype(np.float64), z64), name  # the cast is exact
        assert np.array_equal(z64 * HE.GRID, np.rint(z64 * HE.GRID)), name
    print(f"largest premise {worst:.0f} = 2^{np.log2(worst):.2f}")


def _fp32_chain(terms, b):
    """fp32 accumulation from +0 along the last axis in the order given, one rounding per addition, then the bias."""
    return (np.cumsum(terms, axis=-1, dtype=np.float32)[..., -1] + b).astype(np.float32)


def _fp32_blocks(terms, b):
    """As the MFMA walks k: blocks of 16 terms, each summed as a tree in fp32, the block sums joining one chain; then the bias."""
    K = terms.shape[-1]
    t = np.concatenate((terms, np.zeros(terms.shape[:-1] + (-K % 16,), np.float32)), axis=-1)
    t = t.reshape(t.shape[:-1] + (-1, 16))
    while t.shape[-1] > 1:
        t = (t[..., 0::2] + t[..., 1::2]).astype(np.float32)
    return _fp32_chain(t[..., 0], b)


def test_every_order_of_fp32_additions_gives_want(cases):
    for c, (name, x, w, b) in enumerate(cases):
        f, r = _sample(x, w, b, c)
        terms = (x[f][:, None, :] * w[r][None, :, :]).astype(np.float32)  # products of two halves: exact in fp32
        assert np.array_equal(terms.astype(np.float64), x[f][:, None, :].astype(np.float64) * w[r][None, :, :]), name
        z = HE.want(x[f], w[r], b[r])
        rng = np.random.default_rng(c)
        orders = [np.arange(terms.shape[-1]), np.arange(terms.shape[-1])[::-1]] + [rng.permutation(terms.shape[-1]) for _ in range(3)]
        order_by_size = np.argsort(-np.abs(terms[0, 0]), kind="stable")  # the largest magnitudes first: the largest partial sums
        for p in orders + [order_by_size]:
            assert FR.same_bits(_fp32_chain(terms[..., p], b[r]), z), name
        for p in orders[:3]:
            assert FR.same_bits(_fp32_blocks(terms[..., p], b[r]), z), name


def _every_tile_changes(changed):
    """Has every 32-frame x 32-node tile of the outputs (one MFMA's D, the smallest unit a kernel can get wrong) a changed one?"""
    n, rows = changed.shape
    per_tile = np.add.reduceat(np.add.reduceat(changed.astype(np.int64), np.arange(0, n, 32), axis=0), np.arange(0, rows, 32), axis=1)
    return bool((per_tile > 0).all())


def test_every_planted_fault_changes_the_value(cases):
    """Sensitivity is a condition, not a rate.  A term dropped, a term repeated and the next row's bias change EVERY output,
    by construction (no term is zero, neighbouring biases differ, all arithmetic is exact): held on a sample, for every k.
    The next row's weights and x shifted against w change an output unless two random exact sums coincide, which about one
    output in a thousand does at K = 32; a kernel that makes such a mistake makes it for a whole MFMA tile, so the condition is
    that no 32 x 32 tile of any case is without a changed output -- held on ALL outputs."""
    unchanged = 0
    for c, (name, x, w, b) in enumerate(cases):
        f, r = _sample(x, w, b, c)
        z64 = HE.want64(x[f], w[r], b[r])
        z = z64.astype(np.float32)
        terms = x[f][:, None, :].astype(np.float64) * w[r][None, :, :]  # [frames][rows][K]
        assert ((z64[..., None] - terms).astype(np.float32) != z[..., None]).all(), f"{name}: a term dropped"
        assert ((z64[..., None] + terms).astype(np.float32) != z[..., None]).all(), f"{name}: a term repeated"
        z = HE.want(x, w, b)
        assert (HE.want(x, w, np.roll(b, -1)) != z).all(), f"{name}: the next row's bias"
        faults = {"the next row's weights": HE.want(x, np.roll(w, -1, axis=0), b)}
        for shift in (8, 16):  # half an MFMA step and a whole one
            faults[f"x shifted by {shift} k against w"] = HE.want(np.roll(x, shift, axis=1), w, b)
        for what, zf in faults.items():
            assert _every_tile_changes(zf != z), f"{name}: {what}"
            unchanged += int((zf == z).sum())
    print(f"outputs that a row or k shift leaves unchanged, all cases: {unchanged}")


# ------------------------------------------------------------------------------------------------------------ coverage
def _small_tiles(n, rows, form):
    """(NT, FT) of hsmall_kernel for a layer call, from the plan query: the grid gives the node tile."""
    rp = HE.rows_pad(rows)
    applies, grid, ft = api.half_small_plan(n, 128, rp, 0 if form == "sigmoid" else 1)
    assert applies and rp % (32 * grid) == 0
    return rp // (32 * grid), ft


def test_tables_cover_the_mid_kernel():
    calls = [c for c in HE.layer_calls() if c[1] == "mid"]
    for form, _, K, rows, n in calls:
        applies, ftiles, ntiles = api.half_mid_plan(n, 0, 4096, HE.rows_pad(rows), 0 if form == "sigmoid" else 1)
        assert applies and ftiles == -(-n // 64) and ntiles == HE.rows_pad(rows) // 64
    assert {n for *_, n in calls} == {65, 129}  # a second and a third frame tile of one frame
    for form in ("sigmoid", "exp"):
        kp = sorted({HE.k_pad(K) for f, _, K, _, _ in calls if f == form})
        # the last stage's MFMA steps (fdnn_half_mid.hip:151), after at least two full stages
        last = {(k % MID_K or MID_K) // 16 for k in kp if (k - 1) // MID_K >= 2}
        assert last == {2, 4, 6, 8}, (form, last)
    stages = {-(-HE.k_pad(K) // MID_K) for _, _, K, _, _ in calls}
    assert {1, 2, 3, 4} <= stages and max(stages) >= 5  # no refill, none, the first refill into slot 0, into slot 1, the ring going round
    for form in ("sigmoid", "exp"):  # the refill path s + 2 < stages (fdnn_half_mid.hip:159) in both forms
        assert max(-(-HE.k_pad(K) // MID_K) for f, _, K, _, _ in calls if f == form) >= 2 * MID_RING + 1


def test_tables_cover_the_small_kernel():
    calls = [c for c in HE.layer_calls() if c[1] == "small"]
    residues = {HE.k_pad(K) % SMALL_K for _, _, K, _, _ in calls if HE.k_pad(K) > SMALL_K}
    assert residues == set(range(0, SMALL_K, 32))  # last-stage pair counts 1 .. 7 and the full 8, after a full stage
    longest = {}
    for form, _, K, rows, n in calls:
        nt, ft = _small_tiles(n, rows, form)
        stream = -(-HE.k_pad(K) // SMALL_K) * (nt + ft)  # tiles of the whole k-loop (fdnn_half_small.hip:105-107)
        longest[(nt, ft)] = max(longest.get((nt, ft), 0), stream)
    assert set(longest) == {(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (2, 3), (2, 4)}
    assert all(v > 2 * SMALL_RING for v in longest.values()), longest


def test_tables_cover_the_tiled_and_the_set_kernel():
    steps = {HE.k_pad(K) // TILED_K for _, kernel, K, _, _ in HE.layer_calls() if kernel == "hgemm"}
    assert {1, 2, 3} <= steps and any(s % 2 and s > 3 for s in steps) and any(s % 2 == 0 and s > 3 for s in steps)
    assert max(steps) >= 2048 // TILED_K  # the bench net's width
    widths = {HE.k_pad(H) for H in HE.EXP_H + (HE.EXP_H_WIDE,)}
    assert max(widths) == 2048 and all(api.half_set_plan([0, 33], [0, 33], k, 256)[0] for k in widths)  # the resident-tile kernel serves all
    blocks = {-(-k // SET_K) for k in widths}
    assert {1, 2, 8} <= blocks and any(k % SET_K for k in widths)  # one block, several, the whole image; a short last block
    assert {HE.k_pad(D) - D for D in HE.SIG_D} >= {0, 4, 12, 16}  # live -0 pad columns of W in layer 0


# ------------------------------------------------------------------------------------------------------------ the plain forms
@pytest.mark.parametrize("name", sorted(HE.PLAIN))
def test_plain_nets_keep_signal(name):
    """A float64 forward of the Gaussian nets: before a byte equality of probabilities is trusted to see the hidden k-loops, the
    last hidden layer must tell the frames apart (every sampled frame distinct, the median per-node range at least 0.25)."""
    net, x = HE.plain_net(name), HE.plain_features(name)
    a = (x.astype(np.float64) + net.shift) * net.scale
    for l in net.layers[:-1]:
        a = FR.sigmoid64(a @ l.weights.astype(np.float64).T + l.bias)
    h = a.astype(np.float16)  # what the device stores
    assert len({r.tobytes() for r in h}) == x.shape[0]
    spread = np.median(a.max(axis=0) - a.min(axis=0))
    print(f"{name}: median per-node range {spread:.3f}")
    assert spread >= 0.25
    z = a @ net.layers[-1].weights.astype(np.float64).T + net.layers[-1].bias
    assert np.abs(z).max() < 80.0  # no logit near exp's overflow: the probabilities are finite and carry the logits
