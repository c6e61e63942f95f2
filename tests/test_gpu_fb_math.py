"""The two stated functions of fdnn_fb.hpp on the device: exp_neg and ladd in a trivial kernel (api.fb_math_device) equal the
host's (api.fb_math_ref, held to float64 by tests/test_fb_host.py and swept by tools/exp_sweep.cpp) BYTE FOR BYTE on about a
million inputs each: every exponent of a non-positive argument, the edges -87, -0, 0, -inf and NaN, equal operands and
operands that are +-inf."""
import numpy as np
import pytest

from fast_dnn_amd import api

pytestmark = pytest.mark.gpu
EDGES = np.array([0xc2ae0000, 0xc2ae0001, 0xc2adffff, 0x80000000, 0x00000000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800000, 0x80000001, 0x00000001, 0x3f800000,
                  0x42b00000, 0x7f7fffff, 0xff7fffff, 0xbf800000, 0xc2aeac50], np.uint32)  # -87 and its neighbours, zeros, infinities, NaNs, denormals, ..


def negatives(seed, per_exponent=4000):
    """Every exponent field 0 .. 254 of a non-positive float with random mantissas, all of [-88, -86] in steps, and the edges."""
    rng = np.random.default_rng(seed)
    ex = np.repeat(np.arange(255, dtype=np.uint32), per_exponent)
    bits = np.uint32(0x80000000) | (ex << np.uint32(23)) | rng.integers(0, 1 << 23, ex.size).astype(np.uint32)
    near = np.linspace(-88, -86, 20001).astype(np.float32).view(np.uint32)
    return np.concatenate([bits, near, EDGES]).view(np.float32)


def on_device(op, a, b=None):
    import torch

    d_a = torch.from_numpy(a).cuda()
    d_b = torch.from_numpy(b).cuda() if b is not None else None
    d_out = torch.full((a.size + 8,), -7.0, dtype=torch.float32, device="cuda")
    api.fb_math_device(op, d_a.data_ptr(), d_b.data_ptr() if b is not None else 0, d_out.data_ptr() + 16, a.size)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[:4] == -7).all() and (out[4 + a.size:] == -7).all()
    return out[4:4 + a.size]


def test_exp_neg_on_the_device_has_the_hosts_bytes():
    x = negatives(1)
    assert x.size > 10 ** 6
    want = api.fb_math_ref(api.FB_EXP_NEG, x)
    got = on_device(api.FB_EXP_NEG, x)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (bad.size, x[bad[:5]].view(np.uint32), got[bad[:5]].view(np.uint32), want[bad[:5]].view(np.uint32))
    dom = (x >= -87) & (x <= 0)
    assert dom.sum() > 500000 and (want[dom] >= np.finfo(np.float32).tiny).all() and (want[x < -87].view(np.uint32) == 0).all()  # no denormal; +0 below -87


def test_ladd_on_the_device_has_the_hosts_bytes():
    rng = np.random.default_rng(2)
    d = negatives(3)  # the difference lo - hi, every exponent
    hi = np.concatenate([rng.uniform(-500, 50, d.size - 40000), rng.integers(-40, 5, 40000)]).astype(np.float32)
    with np.errstate(all="ignore"):
        lo = (hi + d).astype(np.float32)
    eq = rng.uniform(-800, 100, 20000).astype(np.float32)  # equal operands
    sp = np.array([-np.inf, np.inf, np.nan, 0.0, -0.0, 1.5, -3e38, 3e38], np.float32)  # every pair of these
    a = np.concatenate([hi, lo, eq, np.repeat(sp, sp.size)])
    b = np.concatenate([lo, hi, eq, np.tile(sp, sp.size)])
    assert a.size > 10 ** 6
    want = api.fb_math_ref(api.FB_LADD, a, b)
    got = on_device(api.FB_LADD, a, b)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (bad.size, a[bad[:5]], b[bad[:5]], got[bad[:5]].view(np.uint32), want[bad[:5]].view(np.uint32))
    ok = ~(np.isnan(a) | np.isnan(b))
    assert (want[ok] >= np.maximum(a[ok], b[ok])).all() and not np.isnan(want[ok]).any()  # >= max, and never a NaN from non-NaNs
    assert (want[~ok].view(np.uint32) == 0x7fc00000).all()


def test_argument_errors():
    with pytest.raises(api.FdnnError):
        api.fb_math_device(2, 0, 0, 0, 4)
    with pytest.raises(api.FdnnError):
        api.fb_math_device(api.FB_LADD, 0, 0, 0, 4)
    api.fb_math_device(api.FB_EXP_NEG, 0, 0, 0, 0)  # nothing to do
