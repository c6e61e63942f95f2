"""A float64 reference for the UNQUANTIZED net (fdnn_float.hip) and the bounds its fp32 results are held to.  numpy only, no GPU.

    u = 2^-24, the unit round-off of fp32;  gamma(m) = m u / (1 - m u)  (Higham, Accuracy and Stability, section 3.1)

Every layer is judged ALONE: the float64 value is taken on the SAME fp32 inputs the device (or the host restatement) was
given, so no bound has to carry the error of the layers before.

1. Sums (lin_bound)
   z = fl(s_K + b), s_k = fl(s_{k-1} + x_k w_k) with ONE rounding per step when fused (fmaf), two when not; in any order.
   The standard result for a recursive sum of K products plus one more addition (Higham, section 3.1, eq. 3.4 / 3.5: each
   term collects at most K + 1 factors (1 + d), |d| <= u, whatever the order and whether or not the products round) is

       |z - z64| <= gamma(K + 1) (sum_k |x_k w_k| + |b|)            while nothing underflows,

   and a product or a partial sum that lands in the subnormal range adds an absolute error of at most 2^-150 < 2^-126 each
   instead of a relative one: K 2^-126 covers all of them generously.  Hence

       bound = gamma(K + 1) (sum_k |x_k w_k| + |b|) + K 2^-126.

   z64 itself (numpy float64 matmul) is off by about K 2^-53 sum|x w|: nine orders below the bound.

2. Input step (exact restatement only; two correctly rounded operations: (x + shift), then * scale -- compared bit for bit).

3. Sigmoid (sigmoid_bound)
   The device computes y = RN(-z L), L = RN32(log2 e); e = exp2(y) (1 + c_e u'); d = RN(1 + e); s = RN(1 / d).
   As in softmax_ref: e = exp(-z) (1 + a), |a| <= (1.23 |z| + c_e) u.  With sigma = 1 / (1 + exp(-z)):
   d sigma / d ln(e) = -sigma (1 - sigma), so the error of e moves s by sigma (1 - sigma) (1.23 |z| + c_e) u; RN(1 + e) and the
   division add one u each, relative to s <= 1: 2 u.  An emulation of the sequence on the CPU with the exp2 off by +-1 ulp,
   over z in [-100, 100], reached 0.75 of the bound with the constant 2; the committed constant is 3:

       |s - sigma64(z)| <= u (sigma (1 - sigma) (1.23 |z| + c_e) + 3),        c_e = softmax_ref.C_E_PATH["exp2.small"].

   The ends: z <= -89 gives y >= 128.4, e = +inf, s = 0 exactly (sigma64 < 2^-128: inside the bound); z >= 104 gives y <= -150,
   e = 0, s = 1 exactly.  Between 87.4 and 104 the hardware exp2 flushes its subnormal result to 0: s = 1, off by < 2^-126.

4. Soft-max: softmax_ref's bound as it stands, on the tap logits z (exact by 1), with DEPTH from rows_pad_of(rows).
"""
import numpy as np

import softmax_ref as SR

U = SR.U
C_E = SR.C_E_PATH["exp2.small"]
SIG_CONST = 3.0


def gamma(m):
    return m * U / (1.0 - m * U)


def lin64(x, w, b):
    """x [n][K] . w [rows][K]^T + b in float64, on the fp32 values given."""
    return np.asarray(x, np.float64) @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)[None, :]


def lin_bound(x, w, b):
    """gamma(K + 1) (sum_k |x_k w_k| + |b|) + K 2^-126 per output (module docstring, 1)."""
    K = np.asarray(w).shape[1]
    S = np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(w, np.float64)).T + np.abs(np.asarray(b, np.float64))[None, :]
    return gamma(K + 1) * S + K * SR.TINY


def lin_failures(z, x, w, b):
    """Outputs of z [n][rows] outside bound 1 -> boolean [n][rows]."""
    z = np.asarray(z)
    assert z.dtype == np.float32
    with np.errstate(invalid="ignore"):
        return ~(np.abs(z.astype(np.float64) - lin64(x, w, b)) <= lin_bound(x, w, b))


def sigmoid64(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


def sigmoid_bound(z):
    s = sigmoid64(z)
    return U * (s * (1.0 - s) * (SR.L_ERR * np.abs(np.asarray(z, np.float64)) + C_E) + SIG_CONST)


def sigmoid_failures(s, z):
    s = np.asarray(s)
    assert s.dtype == np.float32
    return ~(np.abs(s.astype(np.float64) - sigmoid64(z)) <= sigmoid_bound(z))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ fixtures
K_LONG, ROWS_LONG, N_LONG = 2064, 160, 129  # 64 k-steps of 32 plus half a step


def long_k_case(seed=17, c=1.0):
    """The long-k layer: |x_k| and |w_k| / c uniform in [0.75, 1], random signs, so every term lies in [0.5625 c, c] while
    gamma(K + 1) sum|x w| <= 2065 u * 2064 c = 0.254 c = 0.4516 t_min: a result that lacks or repeats ONE term is at least
    t_min - bound > bound away from z64, outside bound 1.  The biases are +-1, +-2, +-3 times c with alternating signs:
    neighbours differ by at least 2 c > 2 bound, |b| <= 3 c adds 3.7e-4 c to the bound."""
    rng = np.random.default_rng(seed)

    def mags(shape):
        return (rng.uniform(0.75, 1.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)

    x = mags((N_LONG, K_LONG))
    w = (mags((ROWS_LONG, K_LONG)) * np.float32(c)).astype(np.float32)
    b = (np.float32(c) * (1 + np.arange(ROWS_LONG) % 3) * np.where(np.arange(ROWS_LONG) % 2, -1.0, 1.0)).astype(np.float32)
    return x, w, b


def planted_faults(x, w, b, layer_ref):
    """name -> z of a restatement with ONE planted fault, each expressed through `layer_ref(w, b, x)` (the library's own
    chain) on doctored operands, so the faulty chains round like the real one."""
    n, K = x.shape
    k = K // 3
    out = {}
    xd = x.copy()
    xd[:, k] = 0.0  # fmaf(0, w, s) = s: the term is gone
    out["one term dropped"] = layer_ref(w, b, xd)
    out["one term doubled"] = layer_ref(np.insert(w, k, w[:, k], axis=1), b, np.insert(x, k, x[:, k], axis=1))
    if K % 32:
        out["the last K mod 32 terms skipped"] = layer_ref(w[:, :K - K % 32], b, x[:, :K - K % 32])
    out["the bias of the neighbouring node"] = layer_ref(w, np.roll(b, 1), x)
    # s starts at the bias: a first term 1 * b, then the bias again at the end as the chain adds it
    out["accumulation started at the bias"] = layer_ref(np.insert(w, 0, b, axis=1), b, np.insert(x, 0, np.float32(1.0), axis=1))
    return out
