"""The float64 lazy soft-max and the relative bound the half net's set step (fdnn_half_set.hip) is held to.  numpy only, no GPU.

For a row with listed logits z_j (len of them) of an output layer of O nodes, every unlisted node has logit 0:
    total = sum_j exp(z_j) + (O - len),   p_j = exp(z_j) / total,   inactive = 1 / total.
The device forms e_j = exp2(RN(z_j RN32(log2 e))) = e^z_j (1 + A_j u'), A_j = 1.23 |z_j| + c_e, exactly as softmax_ref derives
it.  All terms are >= 0, the count O - len is an exact fp32, and the total is len + 1 terms added in SOME order: at most
len + 1 rounded additions lie between a term and the total (the finish kernel's strided lanes and its six exchanges are far
fewer; the bound does not lean on that order), so total' = total (1 + t), |t| <= u (sum_j p_j A_j + len + 1).  inactive is one
IEEE division, p_j one more product:
    |inactive' / inactive - 1| <= u (sum_j p_j A_j + len + 1 + 1),   |p_j' / p_j - 1| <= u (A_j + sum_j p_j A_j + len + 1 + 2).
First order in u = 2^-24, as softmax_ref's bound; it needs every e^z_j and the total to be normal fp32 numbers."""
import numpy as np

import float_ref as FR
import softmax_ref as SR


def lazy64(z, O):
    e = np.exp(np.asarray(z, np.float64))
    total = e.sum(axis=1) + (O - e.shape[1])
    return e / total[:, None], 1.0 / total


def bounds(z, O, c_e=FR.C_E):
    """-> (relative bound of every probability [n][len], of every inactive value [n])."""
    A = SR.L_ERR * np.abs(np.asarray(z, np.float64)) + c_e
    common = (lazy64(z, O)[0] * A).sum(axis=1) + A.shape[1] + 1
    return SR.U * (A + common[:, None] + 2), SR.U * (common + 1)


def check(probs, inactive, z, O, what):
    assert probs.dtype == np.float32 and inactive.dtype == np.float32 and probs.shape == z.shape
    p64, i64 = lazy64(z, O)
    bp, bi = bounds(z, O)
    rp, ri = np.abs(probs / p64 - 1.0), np.abs(inactive / i64 - 1.0)
    assert (rp <= bp).all() and (ri <= bi).all(), f"{what}: worst {float((rp / bp).max()):.3f} / {float((ri / bi).max()):.3f} of the bound"
