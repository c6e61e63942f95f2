"""The bounds the HALF-PRECISION net (fdnn_half.hip) is held to against float64, and its long-k case.  numpy only, no GPU.

Every layer is judged ALONE, on the very fp16 operands the device used: the weights as np.float16 (the loader's round to nearest
even) and the device's own activations of the layer before.

1. Sums.  Products of two halves are exact in fp32; the MFMA adds them in an order that is not documented, so each of the K
   additions (and the bias's) is given one WHOLE fp32 ulp, u' = 2^-23 -- Higham's any-order result (section 3.1) with u'
   in place of u, which also covers an adder that truncates when it aligns the terms inside an instruction:
       |z - z64| <= g'(K + 1) (sum |x w| + |b|) + K 2^-126,   g'(m) = m u' / (1 - m u').
2. Hidden activation.  The fp32 sigmoid sequence's bound (float_ref.sigmoid_bound), one rounding to fp16 (2^-11 relative),
   and half the step of the subnormal halves (2^-25) where the result is below 2^-14.
"""
import numpy as np

import float_ref as FR
import softmax_ref as SR

U1 = 2.0 ** -23


def gamma1(m):
    return m * U1 / (1.0 - m * U1)


def halves(a):
    """fp32 -> the fp32 values of its fp16 roundings."""
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def lin_bound(x, w, b):
    K = np.asarray(w).shape[1]
    S = np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(w, np.float64)).T + np.abs(np.asarray(b, np.float64))[None, :]
    return gamma1(K + 1) * S + K * SR.TINY


def lin_failures(z, x, w, b):
    """Outputs of z [n][rows] outside bound 1, x and w holding fp16 values -> boolean [n][rows]."""
    assert z.dtype == np.float32
    with np.errstate(invalid="ignore"):
        return ~(np.abs(z.astype(np.float64) - FR.lin64(x, w, b)) <= lin_bound(x, w, b))


def act_failures(a, z):
    s = FR.sigmoid64(z)
    assert a.dtype == np.float32 and np.array_equal(a, halves(a))  # the stored values ARE halves
    return ~(np.abs(a.astype(np.float64) - s) <= FR.sigmoid_bound(z) + 2.0 ** -11 * s + 2.0 ** -25)


K_LONG, ROWS_LONG, N_LONG = 1040, 160, 129  # 32 k-steps of 32 plus half a step: the K-pad tail is live


def long_k_case(seed=17):
    """|x_k| and |w_k| uniform in [0.75, 1] with random signs, rounded to fp16 FIRST; biases as float_ref.long_k_case."""
    rng = np.random.default_rng(seed)

    def mags(shape):
        return halves(rng.uniform(0.75, 1.0, shape) * rng.choice([-1.0, 1.0], shape))

    b = ((1 + np.arange(ROWS_LONG) % 3) * np.where(np.arange(ROWS_LONG) % 2, -1.0, 1.0)).astype(np.float32)
    return mags((N_LONG, K_LONG)), mags((ROWS_LONG, K_LONG)), b


def long_k_margin(x, w, b):
    """(largest bound, smallest |x w| term): a lost, repeated or skipped term, or the neighbour's bias (at least 2 away),
    cannot pass while the bound stays below HALF the smallest term."""
    return float(lin_bound(x, w, b).max()), float(np.abs(x).min() * np.abs(w).min())
