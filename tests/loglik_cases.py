"""The planted rows of the decoder-score tests (tests/test_loglik_host.py on the CPU, tests/test_gpu_loglik*.py on the GPU)
and the contract's three steps in numpy, built on api.ln_ref (the ONE logarithm):

    s = ln(p) - log_prior            one fp32 subtraction
    s = floor where s < floor        a NaN stays a NaN
    F16: numpy's float32 -> float16  round to nearest even, denormals kept, |s| >= 65520 -> +-inf

Everything is seeded; rows are float32 arrays whose BITS matter."""
import numpy as np

import topk_cases as TC
from fast_dnn_amd import api

WIDTHS = (1, 3, 4, 5, 63, 64, 65, 251, 1001, 8000)
NS = (1, 5, 130)
TYPES = (api.LOGLIK_F32, api.LOGLIK_F16)
FLOORS = (-np.inf, -20.0)
ROW_KINDS = ("softmax", "special", "below_one", "split", "denormal_border")
SPLIT = 0x3f3504f3  # the mantissa split of ln: sqrt(1/2) rounded up


def priors(width, seed=0):
    """Finite log priors of a soft-max over `width` nodes: about -ln(width), spread by a few nats."""
    rng = np.random.default_rng(77 * width + seed)
    z = (rng.standard_normal(width) * 1.5).astype(np.float64)
    p = np.exp(z - z.max())
    return np.log(p / p.sum()).astype(np.float32)


def rows_of(kind, n, width, seed=0):
    if kind == "softmax":
        return TC.rows_of("softmax", n, width, 1, seed)
    if kind == "special":  # every special bit pattern in every column class
        r = TC.rows_of("special", n, width, 1, seed)
        flat = r.reshape(-1)
        flat[:min(flat.size, TC.SPECIALS.size)] = TC.SPECIALS[:flat.size]
        return r
    total = n * width
    if kind == "below_one":  # consecutive floats below 1 (2^16 of them where the shape has room), 1.0 the last
        start = 0x3f800000 - total + 1
        u = np.arange(start, start + total, dtype=np.int64)
    elif kind == "split":  # the floats around the mantissa split (+-2^12 where the shape has room)
        u = SPLIT - total // 2 + np.arange(total, dtype=np.int64)
    elif kind == "denormal_border":  # the floats around the smallest normal
        u = 0x00800000 - total // 2 + np.arange(total, dtype=np.int64)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(u.astype(np.uint32).view(np.float32).reshape(n, width))


def loglik_numpy(rows, log_prior, floor, type):
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    lp = np.ascontiguousarray(log_prior, dtype=np.float32)
    with np.errstate(all="ignore"):
        s = api.ln_ref(rows) - lp[None, :]
        s = np.where(s < np.float32(floor), np.float32(floor), s).astype(np.float32)
        return s.astype(np.float16) if type == api.LOGLIK_F16 else s


def entries_numpy(nodes, p, log_prior, floor, type):
    nodes = np.asarray(nodes, dtype=np.int64)
    lp = np.ascontiguousarray(log_prior, dtype=np.float32)
    inside = (nodes >= 0) & (nodes < lp.size)
    with np.errstate(all="ignore"):
        s = api.ln_ref(np.asarray(p, np.float32)) - lp[np.where(inside, nodes, 0)]
        s = np.where(s < np.float32(floor), np.float32(floor), s).astype(np.float32)
        s[~inside] = np.nan
        return s.astype(np.float16) if type == api.LOGLIK_F16 else s


def same_bytes(a, b):
    """Byte for byte, except that a NaN matches any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    ua, ub = (a.view(np.uint16), b.view(np.uint16)) if a.dtype == np.float16 else (a.view(np.uint32), b.view(np.uint32))
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (ua[~na] == ub[~nb]).all())


def assert_log_of_rows(dense, lp, s32, s16):
    """Against something independent of the library's logarithm: float64 log of the dense rows minus the priors, within
    kLnMaxUlp (0.85) ulps of ln plus the subtraction's half ulp (fp32 scores `s32`, no floor), and that rounded once more to
    fp16 (`s16`: half an fp16 ulp) -- wherever the row's entry is positive.  -> the largest |s32 - exact| / bound."""
    ok = dense > 0
    s = np.asarray(s32).astype(np.float64)
    exact = np.log(dense.astype(np.float64), where=ok, out=np.zeros(dense.shape)) - lp.astype(np.float64)[None, :]
    ln_ulp = np.spacing(np.abs(np.log(dense.astype(np.float64), where=ok, out=np.ones(dense.shape))).astype(np.float32)).astype(np.float64)
    bound = 0.85 * ln_ulp + 0.5 * np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    assert (np.abs(s - exact)[ok] <= bound[ok]).all()
    h = np.asarray(s16).astype(np.float64)
    assert (np.abs(h - s)[ok] <= 0.5 * np.spacing(np.abs(s).astype(np.float16)).astype(np.float64)[ok] * 1.0000001).all()
    return float((np.abs(s - exact)[ok] / bound[ok]).max()) if ok.any() else 0.0
