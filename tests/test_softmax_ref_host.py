"""tests/softmax_ref.py on the CPU: the float64 reference and its relative bound accept a correctly rounded soft-max and
reject the faults an output epilogue could have -- every one of which (the NaN apart) the suite's `|p - oracle| <= 2e-6`
accepts.  The nets are the ledger's with the output biases on a shuffled ladder over [-40, 20] ('lad/256', 'lad/251',
'ladfull': tests/dispatch_ledger.py), the logits are the oracle's."""
import numpy as np
import pytest

import dispatch_ledger as L
import softmax_ref as SR
from fast_dnn_amd import formats as F
from oracle.oracle import Oracle

NETS = (("lad/256", 33), ("lad/251", 33), ("ladfull", 24))
SMALL = 1e-9  # the planted faults sit on entries below this


class Fixture:
    def __init__(self, kind, n):
        orc = Oracle(L.net_path(kind))
        x = F.synth_features(n, 432, seed=1000 + n)
        self.want, wt = orc.calculate(x, taps=True)  # the oracle's own fp32 soft-max: what today's absolute bar compares with
        self.rows_pad = SR.rows_pad_of(orc.out_dim)
        self.z = SR.logits(wt["acc_out"], SR.coef_of(orc), orc.layer_bias(orc.n_layers - 1), tap=wt["logits"])  # (asserts: bit for bit the tap)
        self.p64 = SR.softmax64(self.z)
        self.good = self.p64.astype(np.float32)
        self.kind = kind
        orc.close()


_FIX = {}


def fixture_of(kind, n):
    if kind not in _FIX:
        _FIX[kind] = Fixture(kind, n)
    return _FIX[kind]


@pytest.fixture(scope="module", params=NETS, ids=[k for k, _ in NETS])
def fx(request):
    return fixture_of(*request.param)


def old_bar_accepts(got, fx):
    try:
        L._softmax_ok(got, fx.want, fx.kind)
        return True
    except AssertionError:
        return False


def rejected(got, fx):
    bad, _ = SR.failures(got, fx.z, fx.rows_pad)
    return bool(bad)


def small_entry(fx, k=0):
    """(row, column) of the k-th entry below SMALL (row-major)."""
    r, c = np.nonzero(fx.p64 < SMALL)
    return r[k], c[k]


def test_fixture_facts_the_gpu_tests_rely_on(fx):
    assert (fx.p64 >= SR.TINY).all(), "a probability of the ladder nets is not a normal fp32"
    assert (fx.p64 < L.TIGHT).mean() > 0.75
    assert fx.z.min() < -39.0 and fx.z.max() > 19.0
    assert (fx.z * np.float32(1.4426950408889634) > -126).all()  # exp's own result is normal too


def test_rounded_float64_passes_within_one_u(fx):
    assert np.abs(SR.rel_err(fx.good, fx.p64)).max() <= SR.U
    assert SR.check(fx.good, fx.z, fx.rows_pad, fx.kind) == 0.0
    assert old_bar_accepts(fx.good, fx)
    m = SR.measure(fx.good, fx.z, fx.rows_pad)
    assert m["min_c_e"] == 0.0 and m["worst_rel_u"] <= 1.0


def test_the_bound_is_the_derived_one(fx):
    """u (A_i + sum_j p_j A_j + DEPTH + 2) with A = 1.23 |z| + c_e: a few 1e-6 on these nets, whatever the probability."""
    b = SR.bound(fx.z, fx.p64, fx.rows_pad)
    A = 1.23 * np.abs(fx.z.astype(np.float64)) + SR.C_E
    i = np.unravel_index(np.argmin(fx.p64), fx.p64.shape)
    assert b[i] == pytest.approx(SR.U * (A[i] + (fx.p64[i[0]] * A[i[0]]).sum() + SR.depth(fx.rows_pad) + 2), rel=1e-12)
    assert SR.depth(256) == 34 and SR.depth(8192) == 39 and SR.depth(33024) == 42
    assert 2e-6 < b.min() and b.max() < 1e-5


def test_masked_out_logits_are_zero(fx):
    masks = F.generate_masks(fx.z.shape[0], fx.z.shape[1], 0.40, 0.03, seed=3)
    orc = Oracle(L.net_path(fx.kind))
    acc = np.rint((fx.z.astype(np.float64))).astype(np.int32)  # any accumulators: the rule under test is the mask's
    z = SR.logits(acc, SR.coef_of(orc), orc.layer_bias(orc.n_layers - 1), masks=masks)
    orc.close()
    assert (z[masks == 0] == 0).all() and z.dtype == np.float32
    p = SR.softmax64(z)
    off = masks[0] == 0
    assert np.ptp(p[0][off]) == 0.0  # exp(0) / total each


# ------------------------------------------------------------------------------------------------------- planted faults
def swap_in_a_group_of_four(fx):
    got = fx.good.copy()
    small = (fx.p64 < SMALL)[:, :fx.p64.shape[1] // 4 * 4].reshape(fx.p64.shape[0], -1, 4)
    r, g = np.argwhere(small.sum(2) >= 2)[0]
    a, b = 4 * g + np.flatnonzero(small[r, g])[:2]
    assert got[r, a] != got[r, b]
    got[r, a], got[r, b] = got[r, b], got[r, a]
    return got


def zero_one(fx):
    got = fx.good.copy()
    got[small_entry(fx, 7)] = 0.0
    return got


def scale_one_by_2_to_minus_12(fx):
    got = fx.good.copy()
    i = small_entry(fx, 11)
    got[i] = np.float32(got[i] * np.float32(1 + 2.0 ** -12))
    return got


def nan_one(fx):
    got = fx.good.copy()
    got[small_entry(fx, 5)] = np.nan
    return got


def row_totals(fx):
    return np.exp(fx.z.astype(np.float64)).sum(1)


def scale_row_by_the_next_rows_total(fx, only_below=np.inf):
    got = fx.good.copy()
    t = row_totals(fx)
    sel = fx.p64[3] < only_below
    got[3][sel] = (fx.p64[3][sel] * t[3] / t[4]).astype(np.float32)
    return got


FAULTS = {"swap_in_a_group_of_four": swap_in_a_group_of_four, "zero_one": zero_one, "scale_one_by_2_to_minus_12": scale_one_by_2_to_minus_12}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_fault_is_rejected_and_invisible_to_the_absolute_bar(fx, fault):
    got = FAULTS[fault](fx)
    assert not np.array_equal(got, fx.good, equal_nan=True)
    assert rejected(got, fx), f"{fault}: check() accepts it"
    with pytest.raises(AssertionError):
        SR.check(got, fx.z, fx.rows_pad, fault)
    assert old_bar_accepts(got, fx), f"{fault}: the 2e-6 absolute bar already sees it"


def test_planted_nan_is_rejected(fx):
    got = nan_one(fx)
    assert rejected(got, fx) and not old_bar_accepts(got, fx)
    # ... and where the oracle has the same NaN, the pattern is the check: the row is outside the bound
    assert not SR.failures(got, fx.z, fx.rows_pad, oracle_nan=np.isnan(got))[0]


def test_row_scaled_by_the_next_rows_total(fx):
    """Frames differ, so their totals do, by per cent: the absolute bar sees this fault through the row's few large entries and
    only through them -- confined to the entries below 2e-6 (more than three quarters of the row) it passes that bar; check()
    rejects both."""
    t = row_totals(fx)
    assert abs(t[3] / t[4] - 1) > 1e-3
    assert rejected(scale_row_by_the_next_rows_total(fx), fx)
    below = scale_row_by_the_next_rows_total(fx, only_below=L.TIGHT)
    assert rejected(below, fx) and old_bar_accepts(below, fx)


def test_flush_below_2_to_minus_100_of_the_row_maximum():
    """No probability of the [-40, 20] ladders is that small (2^-100 = e^-69.3: the flush changes nothing there, asserted), so this
    fault is planted on the underflow net's ladder over [-120, 0]: entries between 2^-126 and 2^-100 of the maximum become 0."""
    for kind, n in NETS:
        f = fixture_of(kind, n)
        assert (f.p64 >= 2.0 ** -100 * f.p64.max(1, keepdims=True)).all()
    fx = fixture_of("tail/und", 33)
    got = fx.good.copy()
    flush = fx.p64 < 2.0 ** -100 * fx.p64.max(1, keepdims=True)
    assert (flush & (fx.p64 >= SR.TINY)).any()
    got[flush] = 0.0
    share = (fx.p64 < SR.TINY).mean()
    assert 0.2 < share < 0.35
    assert SR.check(fx.good, fx.z, fx.rows_pad, "tail/und") == share  # the second class: denormals of float32(p64) are within its rule
    assert rejected(got, fx) and old_bar_accepts(got, fx)
    # every entry below 2^-126 flushed (what v_exp_f32 does) is what the second class allows
    flushed = np.where(fx.p64 < SR.TINY, np.float32(0), fx.good)
    assert SR.check(flushed, fx.z, fx.rows_pad, "tail/und flushed") == share
    # ... and the first class of that net has a normal exp: the GPU tests' premise
    assert (fx.z[fx.p64 >= SR.TINY] * np.float32(1.4426950408889634) > -126).all()


# ------------------------------------------------------------------------------------------- the exp-error estimator
def simulated_pipeline(fx, ulps, seed=0):
    """The library's operations in numpy fp32 -- y = RN(z L), e = exp2(y), a total, e RN(1 / total) -- with an exp2 of known
    error: correctly rounded (at most 1 u), then every result moved `ulps` ulps (2 u each) up or down at random."""
    y = (fx.z * np.float32(1.4426950408889634)).astype(np.float32)
    e = np.exp2(y.astype(np.float64)).astype(np.float32)
    rng = np.random.default_rng(seed)
    for _ in range(ulps):
        e = np.nextafter(e, np.where(rng.random(e.shape) < 0.5, np.float32(0), np.float32(np.inf)).astype(np.float32))
    inv = (np.float32(1) / e.astype(np.float64).sum(1).astype(np.float32)).astype(np.float32)
    return (e * inv[:, None]).astype(np.float32)


@pytest.mark.parametrize("ulps", [0, 1, 2])
def test_measure_brackets_a_known_exp_error(fx, ulps):
    """measure()'s direct estimate, which the committed c_e rests on: exp_err_lower_u never exceeds the planted worst error
    (1 + 2 ulps, in u) and comes within 1 u of it on rows this wide; exp_err_upper_u is that plus the final multiply's u.  The
    issue's 'smallest c_e that passes' is 0 for all three: the derived terms' slack hides an exp that is two ulps off."""
    p = simulated_pipeline(fx, ulps)
    m = SR.measure(p, fx.z, fx.rows_pad)
    worst = 1 + 2 * ulps
    assert worst - 1.0 <= m["exp_err_lower_u"] <= worst, m
    assert m["exp_err_upper_u"] == pytest.approx(m["exp_err_lower_u"] + 1.0)
    assert m["min_c_e"] == 0.0 and not SR.failures(p, fx.z, fx.rows_pad)[0]
