"""The decoder-score kernels alone (fdnn_loglik_rows_device, fdnn_loglik_entries_device; fdnn_loglik.hip) on planted device
rows, on a side stream, against the host restatement (api.loglik_ref; tests/test_loglik_host.py holds that to numpy on the one
logarithm, tests/host/loglik_check.cpp the logarithm to float64): every width at which the kernel takes another path (one
value, odd widths, multiples of 4 that are no multiple of 8, below / at / above a wave, more than one column block, the
8000-node row), n of one row, a few and more than one row block, both types, no floor and a floor, the plan's form, the
vector form where allowed and the scalar-access form.  Byte for byte, NaN against NaN."""
import numpy as np
import pytest

import loglik_cases as LC
import topk_cases as TC
from fast_dnn_amd import api
from guarded import guarded, in_guard, out_guard

pytestmark = pytest.mark.gpu
PAD = 8  # sentinel elements past [n][W]


@pytest.fixture(scope="module")
def torch():
    import torch as t

    yield t
    api.set_loglik_kernel(0)


def out_buffer(torch, count, t):
    """count + PAD elements of the type's size holding a sentinel, as an integer tensor."""
    return torch.full((count + PAD,), -7, dtype=torch.int16 if t == api.LOGLIK_F16 else torch.int32, device="cuda")


def as_scores(d_out, n, width, t):
    got = d_out.cpu().numpy()
    assert (got[n * width:] == -7).all(), "sentinels past [n][W]"
    return got[:n * width].view(np.float16 if t == api.LOGLIK_F16 else np.float32).reshape(n, width).copy()


def run_modes(torch, stream, ll, d_rows_ptr, n, d_out, vector_allowed):
    """The scores under modes 0, 1, 2 on a non-default stream -> [scores [n][W]] x 3; checks which form ran."""
    out, width, t = [], ll.width(), ll.type()
    for mode in (0, 1, 2):
        api.set_loglik_kernel(mode)
        d_out.fill_(-7)
        torch.cuda.synchronize()
        before = api.loglik_launches()
        ll.rows_device(d_rows_ptr, n, d_out.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        after = api.loglik_launches()
        vector = mode != 2 and vector_allowed
        assert tuple(a - b for a, b in zip(after, before)) == ((1, 0, 0) if vector else (0, 1, 0)), (mode, width)
        out.append(as_scores(d_out, n, width, t))
    api.set_loglik_kernel(0)
    return out


@pytest.mark.parametrize("kind", LC.ROW_KINDS)
@pytest.mark.parametrize("width", LC.WIDTHS)
def test_scores_are_the_contracts(torch, width, kind):
    stream = torch.cuda.Stream()
    nmax = max(LC.NS)
    rows = LC.rows_of(kind, nmax, width)
    lp = LC.priors(width)
    d_rows = torch.from_numpy(rows.view(np.int32).copy()).cuda()
    assert d_rows.data_ptr() % 16 == 0
    for t in LC.TYPES:
        d_out = out_buffer(torch, nmax * width, t)
        assert d_out.data_ptr() % 16 == 0
        for floor in LC.FLOORS:
            want = api.loglik_ref(rows, lp, floor, t)  # (s is a function of the row and the handle alone: one reference for every n)
            ll = api.Loglik(lp, floor, t)
            assert (ll.width(), ll.type()) == (width, t)
            for n in LC.NS:
                for mode, got in enumerate(run_modes(torch, stream, ll, d_rows.data_ptr(), n, d_out, width % 4 == 0)):
                    assert LC.same_bytes(got, want[:n]), (kind, width, t, floor, n, mode)
            if np.isfinite(floor):
                assert not np.isneginf(want).any()
            ll.delete()
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint32), rows.view(np.uint32)), "the input is unchanged"


@pytest.mark.parametrize("kind,n,width", [("below_one", 64, 1024), ("below_one", 65, 1009), ("split", 8, 1024), ("split", 9, 911),
                                          ("denormal_border", 8, 1024), ("denormal_border", 7, 1171), ("special", 4, 16)])
def test_the_logarithms_seams(torch, kind, n, width):
    """2^16 consecutive floats below 1 (ln x -> -0 side of 0), +-2^12 floats around the mantissa split 0x3f3504f3, the floats
    around the smallest normal 0x00800000 (the 2^24 step), and every special bit pattern in a vector thread's columns."""
    stream = torch.cuda.Stream()
    rows = LC.rows_of(kind, n, width)
    u = rows.view(np.uint32)
    if kind == "below_one":
        assert u.size >= 1 << 16 and u.max() == 0x3f800000 and (np.diff(u.ravel().astype(np.int64)) == 1).all()
    elif kind == "split":
        assert u.min() <= LC.SPLIT - (1 << 12) and u.max() >= LC.SPLIT + (1 << 12) - 1
    elif kind == "denormal_border":
        assert u.min() < 0x00800000 - 4000 and u.max() > 0x00800000 + 4000
    lp = LC.priors(width, seed=1)
    d_rows = torch.from_numpy(rows.view(np.int32).copy()).cuda()
    for t in LC.TYPES:
        d_out = out_buffer(torch, n * width, t)
        for floor in LC.FLOORS:
            ll = api.Loglik(lp, floor, t)
            want = api.loglik_ref(rows, lp, floor, t)
            for mode, got in enumerate(run_modes(torch, stream, ll, d_rows.data_ptr(), n, d_out, width % 4 == 0)):
                assert LC.same_bytes(got, want), (kind, t, floor, mode)
            ll.delete()
    zero = api.Loglik(np.zeros(width, np.float32), -np.inf, api.LOGLIK_F32)  # the logarithm itself: ln_ref, bit for bit
    d_out = out_buffer(torch, n * width, api.LOGLIK_F32)
    zero.rows_device(d_rows.data_ptr(), n, d_out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    with np.errstate(all="ignore"):
        ln = api.ln_ref(rows)
        assert LC.same_bytes(as_scores(d_out, n, width, api.LOGLIK_F32), (ln - np.float32(0)).astype(np.float32))
    zero.delete()


@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("width", [1001, 1004])
def test_bases_off_alignment(torch, shift, width):
    """The input starts 1 to 3 elements past a 16-byte boundary, and so does the output (2, 4, 6 bytes for fp16): a slice of a
    caller's tensor.  The scalar-access form runs whatever the mode."""
    stream = torch.cuda.Stream()
    n = 5
    rows = LC.rows_of("softmax", n, width, seed=shift)
    rows[1] = LC.rows_of("special", 1, width)[0]
    lp = LC.priors(width)
    flat = np.concatenate([np.zeros(shift, np.float32), rows.ravel(), np.zeros(4, np.float32)])
    d_all = torch.from_numpy(flat.view(np.int32).copy()).cuda()
    d_aligned = torch.from_numpy(rows.view(np.int32).copy()).cuda()
    assert d_all.data_ptr() % 16 == 0 and d_aligned.data_ptr() % 16 == 0
    off, aligned = d_all.data_ptr() + 4 * shift, d_aligned.data_ptr()
    for t in LC.TYPES:
        ll = api.Loglik(lp, -20.0, t)
        want = api.loglik_ref(rows, lp, -20.0, t)
        whole = out_buffer(torch, n * width + shift, t)
        out_off, out_aligned = whole[shift:], whole[:n * width + PAD]
        assert out_off.data_ptr() % 16 == shift * (2 if t == api.LOGLIK_F16 else 4) and out_aligned.data_ptr() % 16 == 0
        for src, dst in ((off, out_off), (aligned, out_off), (off, out_aligned)):  # both off, the output alone, the input alone
            whole.fill_(-7)
            for got in run_modes(torch, stream, ll, src, n, dst, False):
                assert LC.same_bytes(got, want), (t, shift)
            if dst is out_off:
                assert (whole[:shift].cpu().numpy() == -7).all(), "the elements before the view"
        ll.delete()
    assert np.array_equal(d_all.cpu().numpy().view(np.uint32), flat.view(np.uint32))


@pytest.mark.parametrize("width,n", [(251, 8), (8000, 6), (1004, 18), (64, 33), (3, 8)])
def test_guarded_buffers(torch, width, n):
    """Every element of the output is written, nothing around it is, and the input allocation keeps its bytes, with poison
    (NaN) around the rows that no result may meet.  (fp16 scores are watched two to a 32-bit word: n x W is even here.)"""
    rows = LC.rows_of("softmax", n, width, seed=3)
    lp = LC.priors(width)
    head, tail = in_guard(width)
    assert n * width % 2 == 0
    for t in LC.TYPES:
        ll = api.Loglik(lp, -20.0, t)
        want = api.loglik_ref(rows, lp, -20.0, t)
        words = n * width if t == api.LOGLIK_F32 else n * width // 2
        for mode in (0, 1, 2):
            for offset in (0, 4):
                api.set_loglik_kernel(mode)
                g_in = guarded(torch.from_numpy(rows).cuda(), torch.float32, head, min(tail, 4 * width), byte_offset=offset, fill=float("nan"), name="d_rows")
                g_out = guarded(words, torch.int32, out_guard(width) // 64, out_guard(width) // 64, byte_offset=offset, device="cuda", name="d_out")
                ll.rows_device(g_in.ptr, n, g_out.ptr)
                torch.cuda.synchronize()
                g_in.check(f"mode {mode}")
                g_out.check(f"mode {mode}")
                got = g_out.view.cpu().numpy().view(np.float16 if t == api.LOGLIK_F16 else np.float32).reshape(n, width)
                assert LC.same_bytes(got, want), (t, mode, offset)
        api.set_loglik_kernel(0)
        ll.delete()


@pytest.mark.parametrize("count", [1, 63, 64, 65, 1000])
def test_entries(torch, count):
    stream = torch.cuda.Stream()
    width = 251
    lp = LC.priors(width)
    rng = np.random.default_rng(count)
    nodes = rng.integers(0, width, count).astype(np.int32)
    p = LC.rows_of("softmax", 4, 250).ravel()[:count].copy()
    p[:min(count, TC.SPECIALS.size)] = TC.SPECIALS[:count]
    if count >= 63:
        nodes[[5, 40, 62]] = (-1, width, np.iinfo(np.int32).min)
    else:
        nodes[0] = -1
    d_nodes = torch.from_numpy(nodes).cuda()
    d_p = torch.from_numpy(p.view(np.int32).copy()).cuda()
    for t in LC.TYPES:
        for floor in LC.FLOORS:
            ll = api.Loglik(lp, floor, t)
            d_out = out_buffer(torch, count, t)
            torch.cuda.synchronize()
            before = api.loglik_launches()
            ll.entries_device(d_nodes.data_ptr(), d_p.data_ptr(), count, d_out.data_ptr(), stream.cuda_stream)
            stream.synchronize()
            after = api.loglik_launches()
            assert tuple(a - b for a, b in zip(after, before)) == (0, 0, 1)
            got = as_scores(d_out, 1, count, t)[0]
            assert LC.same_bytes(got, api.loglik_entries_ref(nodes, p, lp, floor, t)), (count, t, floor)
            assert np.isnan(got[(nodes < 0) | (nodes >= width)]).all()
            ll.delete()


def test_entries_composed_on_the_topk_selection(torch):
    """fdnn_topk_rows_device's (nodes, values) turned into decoder scores on the device: the scores of the k most probable
    nodes of every frame -- which are not the k best scores (include/fdnn.h)."""
    n, width, k = 33, 8000, 5
    rows = TC.rows_of("softmax", n, width, 1, seed=9)
    lp = LC.priors(width)
    d_rows = torch.from_numpy(rows).cuda()
    d_nodes = torch.empty(n * k, dtype=torch.int32, device="cuda")
    d_vals = torch.empty(n * k, dtype=torch.float32, device="cuda")
    api.topk_rows_device(d_rows.data_ptr(), n, width, k, d_nodes.data_ptr(), d_vals.data_ptr())
    want_nodes, want_vals = TC.select(rows, k)
    for t in LC.TYPES:
        ll = api.Loglik(lp, -20.0, t)
        d_out = out_buffer(torch, n * k, t)
        ll.entries_device(d_nodes.data_ptr(), d_vals.data_ptr(), n * k, d_out.data_ptr())
        torch.cuda.synchronize()
        got = as_scores(d_out, n, k, t)
        assert LC.same_bytes(got.ravel(), api.loglik_entries_ref(want_nodes.ravel(), want_vals.view(np.float32).ravel(), lp, -20.0, t))
        full = api.loglik_ref(rows, lp, -20.0, t)  # ... and they are the full row's scores at those nodes
        assert LC.same_bytes(got, np.take_along_axis(full, want_nodes.astype(np.int64), axis=1))
        ll.delete()


def test_argument_errors_launch_nothing(torch):
    for lp, floor, t in (([0.0, np.inf], -np.inf, 0), ([0.0, 0.0], np.nan, 0), ([0.0, 0.0], np.inf, 1), ([0.0, 0.0], -65505.0, 1), ([0.0, 0.0], 0.0, 2)):
        with pytest.raises(api.FdnnError) as e:
            api.Loglik(np.array(lp, np.float32), floor, t)
        assert e.value.code == api.FDNN_E_ARG
    with pytest.raises(api.FdnnError):
        api.Loglik(np.zeros(0, np.float32))
    ll = api.Loglik(np.zeros(100, np.float32), -65504.0, api.LOGLIK_F16)
    d = torch.full((4 * 100,), 0.5, dtype=torch.float32, device="cuda")
    dn = torch.zeros(8, dtype=torch.int32, device="cuda")
    dq = torch.full((4 * 100,), -7, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    before = api.loglik_launches()
    for n, rows_ptr, out_ptr in ((-1, d.data_ptr(), dq.data_ptr()), (4, 0, dq.data_ptr()), (4, d.data_ptr(), 0), (4, d.data_ptr() + 2, dq.data_ptr()),
                                 (4, d.data_ptr(), dq.data_ptr() + 1)):
        with pytest.raises(api.FdnnError) as e:
            ll.rows_device(rows_ptr, n, out_ptr)
        assert e.value.code == api.FDNN_E_ARG, n
    for cnt, np_, pp, op in ((-1, dn.data_ptr(), d.data_ptr(), dq.data_ptr()), (8, 0, d.data_ptr(), dq.data_ptr()), (8, dn.data_ptr(), 0, dq.data_ptr()),
                             (8, dn.data_ptr(), d.data_ptr(), 0)):
        with pytest.raises(api.FdnnError) as e:
            ll.entries_device(np_, pp, cnt, op)
        assert e.value.code == api.FDNN_E_ARG, cnt
    ll.rows_device(d.data_ptr(), 0, dq.data_ptr())  # n == 0: a no-op
    ll.entries_device(dn.data_ptr(), d.data_ptr(), 0, dq.data_ptr())
    torch.cuda.synchronize()
    assert api.loglik_launches() == before and (dq == -7).all()
    ll.delete()
