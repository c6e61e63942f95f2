"""The top-k selection alone (fdnn_topk_rows_device, fdnn_topk.hip) on planted device rows: every width at which the kernel
takes another path (one value, below / at / above a wave, odd widths whose rows start off 16-byte alignment, the 8000-node
row, the widest resident row and the first streaming one), every row kind of tests/topk_cases.py, n of one row, a few and more
than one round of workgroups; the plan's form, the resident form and the streaming form return the same bytes, which are the
contract's stated in numpy on the same array."""
import numpy as np
import pytest

import topk_cases as TC
from fast_dnn_amd import api

pytestmark = pytest.mark.gpu
RW = api.TOPK_RESIDENT_WIDTH
PAD = 8  # sentinel words past [n][k]


@pytest.fixture(scope="module")
def torch():
    import torch as t

    yield t
    api.set_topk_kernel(0)


def run_modes(torch, stream, d_rows_ptr, n, width, k, d_nodes, d_vals):
    """The selection under modes 0, 1, 2 on a non-default stream -> [(nodes, vals as uint32)] x 3; checks which form ran."""
    out = []
    for mode in (0, 1, 2):
        api.set_topk_kernel(mode)
        d_nodes.fill_(-7)
        d_vals.fill_(-7.0)
        torch.cuda.synchronize()
        before = api.topk_launches()
        api.topk_rows_device(d_rows_ptr, n, width, k, d_nodes.data_ptr(), d_vals.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        after = api.topk_launches()
        resident = mode != 2 and width <= RW
        assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if resident else (0, 1)), (mode, width)
        nodes, vals = d_nodes.cpu().numpy(), d_vals.cpu().numpy().view(np.uint32)
        assert (nodes[n * k:] == -7).all() and (vals[n * k:] == np.float32(-7.0).view(np.uint32)).all(), "sentinels past [n][k]"
        out.append((nodes[:n * k].reshape(n, k), vals[:n * k].reshape(n, k)))
    api.set_topk_kernel(0)
    return out


@pytest.mark.parametrize("kind", TC.KINDS)
@pytest.mark.parametrize("width", TC.WIDTHS)
def test_selection_is_the_contracts(torch, width, kind):
    stream = torch.cuda.Stream()
    nmax = max(TC.NS)
    rows = d_rows = want = None
    for k in TC.ks_for(width):
        if rows is None or kind == "plateau":
            rows = TC.rows_of(kind, nmax, width, k)
            d_rows = torch.from_numpy(rows.view(np.int32).copy()).cuda()
            want = TC.select(rows, min(width, api.TOPK_MAX_K))  # (the top k is its prefix: test_topk_host.py)
        d_nodes = torch.empty(nmax * k + PAD, dtype=torch.int32, device="cuda")
        d_vals = torch.empty(nmax * k + PAD, dtype=torch.float32, device="cuda")
        for n in TC.NS:
            got = run_modes(torch, stream, d_rows.data_ptr(), n, width, k, d_nodes, d_vals)
            for mode, (nodes, vals) in enumerate(got):
                assert np.array_equal(nodes, want[0][:n, :k]), (kind, width, n, k, mode)
                assert np.array_equal(vals, want[1][:n, :k]), (kind, width, n, k, mode)
            if kind == "equal":
                assert (got[0][0] == np.arange(k)[None, :]).all()
        assert np.array_equal(d_rows.cpu().numpy().view(np.uint32), rows.view(np.uint32)), "the input is unchanged"


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_rows_whose_base_is_off_alignment(torch, shift):
    """The buffer itself starts 4, 8 or 12 bytes past a 16-byte boundary (a slice of a caller's tensor)."""
    stream = torch.cuda.Stream()
    n, width, k = 5, 1001, 65
    rows = TC.rows_of("softmax", n, width, k, seed=shift)
    rows[1] = TC.rows_of("special", 1, width, k)[0]
    flat = np.concatenate([np.zeros(shift, np.float32), rows.ravel(), np.zeros(4, np.float32)])
    d_all = torch.from_numpy(flat.view(np.int32).copy()).cuda()
    assert d_all.data_ptr() % 16 == 0
    d_nodes = torch.empty(n * k + PAD, dtype=torch.int32, device="cuda")
    d_vals = torch.empty(n * k + PAD, dtype=torch.float32, device="cuda")
    want = TC.select(rows, k)
    for nodes, vals in run_modes(torch, stream, d_all.data_ptr() + 4 * shift, n, width, k, d_nodes, d_vals):
        assert np.array_equal(nodes, want[0]) and np.array_equal(vals, want[1])
    assert np.array_equal(d_all.cpu().numpy().view(np.uint32), flat.view(np.uint32))


def test_argument_errors_launch_nothing(torch):
    d = torch.zeros(4 * 100, dtype=torch.float32, device="cuda")
    dn = torch.full((4 * 100,), -7, dtype=torch.int32, device="cuda")
    dv = torch.full((4 * 100,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    before = api.topk_launches()
    for n, width, k, p in ((4, 100, 0, (d, dn, dv)), (4, 100, 101, (d, dn, dv)), (4, 1000, 257, (d, dn, dv)), (4, 0, 1, (d, dn, dv)), (-1, 100, 1, (d, dn, dv)),
                           (4, 100, 5, (None, dn, dv)), (4, 100, 5, (d, None, dv)), (4, 100, 5, (d, dn, None))):
        ptr = [t.data_ptr() if t is not None else 0 for t in p]
        with pytest.raises(api.FdnnError) as e:
            api.topk_rows_device(ptr[0], n, width, k, ptr[1], ptr[2])
        assert e.value.code == api.FDNN_E_ARG, (n, width, k)
    api.topk_rows_device(d.data_ptr(), 0, 100, 5, dn.data_ptr(), dv.data_ptr())  # n == 0: a no-op
    torch.cuda.synchronize()
    assert api.topk_launches() == before and (dn == -7).all() and (dv == -7.0).all()
