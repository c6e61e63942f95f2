"""A float64 reference for the soft-max and the relative bound the library's fp32 soft-max is held to.  numpy only, no GPU.

The oracle (oracle/fdnn_oracle.c) restates the reference's own fp32 soft-max -- glibc expf, a sequential fp32 row total --
and the suite's `|p - oracle| <= 2e-6` says nothing about a probability below 2e-6: in an 8000-wide row that is most of
them.  This module compares with exp(z - max) / sum in float64 instead, relatively, element by element.

    z = logits(acc, coef, bias, masks)   the reference's fp32 logits, rebuilt bit for bit from oracle state
    p64 = softmax64(z)
    check(got, z, rows_pad, what)        |got / p64 - 1| <= bound(z, p64, rows_pad) wherever p64 is a normal fp32

The bound (first order in u = 2^-24, the unit round-off of fp32; the second-order terms are below 1e-5 of it)
-----------------------------------------------------------------------------------------------------------
Every output path of the library performs, per element i of a row (fdnn_gemm.hip, fdnn_small.hip, fdnn_ppo.hip):

  y_i = RN(z_i * L),  L = RN32(log2 e) = 0x3fb8aa3b.   L is 0.2247 u below log2 e (relative), the product rounds once:
        y_i = z_i log2(e) (1 + d), |d| <= 1.2247 u, hence 2^y_i = e^z_i (1 + a), |a| <= |z_i| |d| <= 1.23 |z_i| u.
  e_i = v_exp_f32(y_i) = 2^y_i (1 + b), |b| <= c_e u: the hardware's exp2.  c_e is the one term with no derivation
        (see C_E below).  Together e_i = e^z_i (1 + A_i u'), |u'| <= u, with

        A_i = 1.23 |z_i| + c_e.

  total: the e_j of a row are added in one fixed order (psum in fdnn_gemm.hip:967 / :977, ps in fdnn_small.hip:371-382, the
        running sum of PPO_EXP4 in fdnn_ppo.hip:232-233; normalize_row, fdnn_kernels.hip:25-60): inside a 64-node partial each
        lane half adds its 32 values one after the other (31 rounded additions: the first lands on 0), the two halves
        are added (1), the four partials of a 256-node tile pairwise (2 levels), the MT = rows_pad / 256 tiles as a
        binary tree (ceil(log2 MT) levels).  All terms are >= 0, so every rounded addition on the way from a leaf to
        the root costs at most u relative to the running sum, and the total's own relative error is at most the
        p-weighted mean of its terms' errors plus one u per addition on the longest leaf-to-root path:

        total' = total (1 + t), |t| <= u (sum_j p_j A_j + DEPTH),   DEPTH = 31 + 1 + 2 + ceil(log2(rows_pad / 256)).

        (A balanced tree over rows_pad leaves would have ceil(log2 rows_pad) levels; the 32-long chains make it
        26 + ceil(log2 rows_pad).  Zero padding adds x + 0 = x, exact.)
  p_i = RN(e_i * RN(1 / total')): the division is IEEE (correctly rounded), the product rounds once: 2 u.

  bound_i = u (A_i + sum_j p_j A_j + DEPTH + 2)

All of this needs every intermediate to be a normal fp32.  v_exp_f32 returns 0 for results below 2^-126 and fp32
multiplies may round into the denormals, so an element whose float64 probability is below 2^-126 is held to the second
rule of check(): zero, or the bound plus one denormal step.  Callers choose logits for which e^z itself stays normal
wherever p64 does (z >= -87.3: total >= 1).  Rows whose fp32 total overflows, or whose oracle row carries a NaN, are
outside the bound: check() compares their NaN pattern and callers compare them with the oracle exactly.
"""
import numpy as np

U = 2.0 ** -24          # unit round-off of fp32
TINY = 2.0 ** -126      # smallest normal fp32
DENORM = 2.0 ** -149    # smallest fp32 denormal
L_ERR = 1.23            # (1 + 0.2247) rounded up: y = RN(z * RN32(log2 e))

# c_e per exp path, in units of u: twice the value measured on an MI355X over the range cases of
# tests/test_gpu_softmax_range.py, rounded up (profiles/LABBOOK.md, "Soft-max: c_e per exp path": measured 0.77, 1.02, 0.77, 0.98).
C_E_PATH = {"expf": 2, "exp2.packed": 3, "exp2.small": 2, "v_exp.ppo": 2}
C_E = max(C_E_PATH.values())


def rows_pad_of(rows):
    """Output rows padded to whole 256-node tiles, as the library pads them."""
    return -(-int(rows) // 256) * 256


def depth(rows_pad):
    """Rounded additions on the longest path from an element to its row total (see the module docstring)."""
    assert rows_pad % 256 == 0 and rows_pad > 0
    return 31 + 1 + 2 + int(np.ceil(np.log2(rows_pad // 256)))


def coef_of(orc):
    """The output layer's divisor as the reference forms it: f32(mult * 255) (dnn.cc:298-299)."""
    return np.float32(np.float32(orc.layer_mult(orc.n_layers - 1)) * np.float32(255.0))


def logits(acc, coef, bias, masks=None, tap=None):
    """The reference's fp32 logits from the int32 output accumulators: f32(f32(acc) / coef) + bias (dnn.cc:311, :446);
    masked-out nodes keep z = 0 (dnn.cc:366-369).  Where the oracle's `logits` tap is given, the two must agree bit for bit."""
    acc = np.asarray(acc)
    assert acc.dtype == np.int32
    z = (acc.astype(np.float32) / np.float32(coef)).astype(np.float32) + np.asarray(bias, dtype=np.float32)[None, :]
    assert z.dtype == np.float32
    if tap is not None:
        assert np.array_equal(z.view(np.uint32), np.asarray(tap, dtype=np.float32).view(np.uint32)), "rebuilt logits differ from the oracle's tap"
    if masks is not None:
        z = np.where(np.asarray(masks) != 0, z, np.float32(0.0)).astype(np.float32)
    return z


def softmax64(z):
    """exp(z - max) / sum per row, in float64."""
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def bound(z, p64, rows_pad, c_e=C_E):
    """Allowed relative error per element: u (A_i + sum_j p_j A_j + DEPTH + 2), A = 1.23 |z| + c_e (module docstring)."""
    A = L_ERR * np.abs(np.asarray(z, dtype=np.float64)) + c_e
    return U * (A + (p64 * A).sum(axis=1, keepdims=True) + depth(rows_pad) + 2)


def rel_err(got, p64):
    """got / p64 - 1 per element (float64)."""
    return np.asarray(got, dtype=np.float64) / p64 - 1.0


def failures(got, z, rows_pad, oracle_nan=None, c_e=C_E):
    """-> (list of what is wrong, share of entries in the second class).  check() asserts the list empty."""
    got = np.asarray(got)
    z = np.asarray(z)
    assert got.dtype == np.float32 and got.shape == z.shape and got.ndim == 2
    bad, n_second = [], 0
    want_nan = np.zeros(got.shape, bool) if oracle_nan is None else np.asarray(oracle_nan, bool)
    if not np.array_equal(np.isnan(got), want_nan):
        bad.append(f"NaN pattern differs from the oracle ({int(np.isnan(got).sum())} NaN, {int(want_nan.sum())} expected)")
    for lo in range(0, got.shape[0], 4096):  # (row blocks: the float64 temporaries of a 65 000-row case stay small)
        sl = slice(lo, lo + 4096)
        g, zb = got[sl].astype(np.float64), z[sl]
        rows = ~(want_nan[sl].any(axis=1) | np.isnan(g).any(axis=1))  # a row with a NaN is outside the bound: its pattern is the check
        p64 = softmax64(zb)
        b = bound(zb, p64, rows_pad, c_e)
        first = (p64 >= TINY) & rows[:, None]
        second = (p64 < TINY) & rows[:, None]
        n_second += int(second.sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.abs(g / p64 - 1.0)
        miss = first & ~(r <= b)
        if miss.any() and len(bad) < 4:
            i = np.unravel_index(np.argmax(np.where(miss, r / b, 0.0)), r.shape)
            bad.append(f"{int(miss.sum())} entries outside the relative bound; worst at ({lo + i[0]}, {i[1]}): p64 {p64[i]:.6e} got {g[i]:.6e} "
                       f"rel {r[i] / U:.1f} u, bound {b[i] / U:.1f} u (z {float(zb[i]):.4f})")
        miss2 = second & ~((g >= 0) & (g <= TINY) & ((g == 0) | (np.abs(g - p64) <= b * p64 + DENORM)))
        if miss2.any() and len(bad) < 4:
            i = np.unravel_index(np.argmax(miss2), miss2.shape)
            bad.append(f"{int(miss2.sum())} entries below 2^-126 are neither 0 nor within the bound; first at ({lo + i[0]}, {i[1]}): "
                       f"p64 {p64[i]:.6e} got {g[i]:.6e}")
    return bad, n_second / max(1, got.size)


def check(got, z, rows_pad, what, oracle_nan=None, c_e=C_E):
    """The NaN pattern equals the oracle's (none unless `oracle_nan` is given); where p64 >= 2^-126, |got / p64 - 1| <= bound;
    where p64 < 2^-126, 0 <= got <= 2^-126 and got is 0 or within bound * p64 + 2^-149.  Returns the share of entries in
    that second class, for callers to cap."""
    bad, share = failures(got, z, rows_pad, oracle_nan, c_e)
    assert not bad, f"{what}: " + "; ".join(bad)
    return share


def measure(got, z, rows_pad):
    """Figures for the lab book, from one result: the worst relative error in u, the smallest c_e (>= 0) for which
    check() passes, and a direct estimate of the exp's own error.  The direct estimate divides got_i by the EXACT
    2^y_i, y_i = RN32(z_i * L) -- so the rounding of y and the 1.23 |z| term drop out -- which leaves
    (1 + exp error_i) * RN(1 / total) * (1 + final rounding_i): one factor per row, times per-element errors.  Half the
    spread of that ratio over a row, minus the final multiply's u, is a lower bound of the largest exp error in the row."""
    got = np.asarray(got)
    zz = np.asarray(z, dtype=np.float32)
    p64 = softmax64(zz)
    g = got.astype(np.float64)
    ok = (p64 >= TINY) & ~np.isnan(g).any(axis=1)[:, None]
    r = np.where(ok, np.abs(g / p64 - 1.0), 0.0)
    b0 = bound(zz, p64, rows_pad, 0.0)
    need = np.where(ok, (r - b0) / U / (1.0 + p64.sum(axis=1, keepdims=True)), -np.inf)  # bound is linear in c_e: slope u (1 + sum p)
    y = (zz * np.float32(1.44269504088896340736)).astype(np.float32)
    ratio = np.where(ok, g / np.exp2(y.astype(np.float64)), np.nan)
    hi, lo = np.nanmax(ratio, axis=1), np.nanmin(ratio, axis=1)
    spread = (hi - lo) / (hi + lo)  # half the spread, relative to the middle
    return {"worst_rel_u": float(r.max() / U), "worst_rel_over_bound0": float(np.where(ok, r / b0, 0.0).max()),
            "min_c_e": float(max(0.0, need.max())), "exp_err_lower_u": float(max(0.0, spread.max() / U - 1.0)),
            "exp_err_upper_u": float(spread.max() / U)}


# ------------------------------------------------------------------------------------------------------------ fixtures
def ladder(width, lo, hi, seed):
    """A shuffled linspace(lo, hi, width) as fp32 output biases: the logits then span exp's range whatever the net computes."""
    b = np.linspace(lo, hi, width).astype(np.float32)
    np.random.default_rng(seed).shuffle(b)
    return b
