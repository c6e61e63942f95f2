"""The class pooling alone (fdnn_pool_rows_device, fdnn_pool.hip) on planted device rows, against the host restatement
(api.pool_ref; tests/test_pool_host.py holds that to numpy and float64): every width at which the kernel takes another path
(one value, below / at / above a wave, odd widths whose rows start off 16-byte alignment, the 8000-node row, the widest
resident row, the first streaming one and the loader's widest), every row kind of tests/topk_cases.py, every map kind of
tests/pool_cases.py, n of one row, a few and more than one workgroup per CU slot; the plan's form, the resident form and the
streaming form return the same bytes.  Byte for byte, NaN against NaN."""
import numpy as np
import pytest

import pool_cases as PC
import topk_cases as TC
from fast_dnn_amd import api
from guarded import guarded, in_guard, out_guard

pytestmark = pytest.mark.gpu
RW = api.POOL_RESIDENT_WIDTH
WIDEST = 1 << 19
WIDTHS = (1, 2, 63, 64, 65, 251, 1001, 8000, RW, RW + 1, WIDEST)
PAD = 8  # sentinel words past [n][C]


@pytest.fixture(scope="module")
def torch():
    import torch as t

    yield t
    api.set_pool_kernel(0)


def ns_of(width):
    return (1, 2) if width == WIDEST else TC.NS


def run_modes(torch, stream, pool, d_rows_ptr, n, d_out):
    """The pooling under modes 0, 1, 2 on a non-default stream -> [float32 [n][C]] x 3; checks which form ran."""
    out, C, width = [], pool.classes(), pool.width()
    for mode in (0, 1, 2):
        api.set_pool_kernel(mode)
        d_out.fill_(-7.0)
        torch.cuda.synchronize()
        before = api.pool_launches()
        pool.rows_device(d_rows_ptr, n, d_out.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        after = api.pool_launches()
        resident = mode != 2 and width <= RW
        assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if resident else (0, 1)), (mode, width)
        got = d_out.cpu().numpy()
        assert (got[n * C:] == np.float32(-7.0)).all(), "sentinels past [n][C]"
        out.append(got[:n * C].reshape(n, C).copy())
    api.set_pool_kernel(0)
    return out


@pytest.mark.parametrize("kind", TC.KINDS)
@pytest.mark.parametrize("width", WIDTHS)
def test_pooling_is_the_contracts(torch, width, kind):
    stream = torch.cuda.Stream()
    nmax = max(ns_of(width))
    rows = TC.rows_of(kind, nmax, width, 1)
    d_rows = torch.from_numpy(rows.view(np.int32).copy()).cuda()
    for mk in PC.MAP_KINDS:
        co, C = PC.map_of(mk, width)
        want = api.pool_ref(rows, co, C)  # (q[r][c] is a function of the row and the map alone: one reference for every n)
        pool = api.ClassPool(co, C)
        assert (pool.width(), pool.classes()) == (width, C)
        d_out = torch.empty(nmax * C + PAD, dtype=torch.float32, device="cuda")
        for n in ns_of(width):
            for mode, got in enumerate(run_modes(torch, stream, pool, d_rows.data_ptr(), n, d_out)):
                assert PC.same_bytes(got, want[:n]), (kind, width, mk, n, mode)
        pool.delete()
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint32), rows.view(np.uint32)), "the input is unchanged"


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_rows_whose_base_is_off_alignment(torch, shift):
    """The buffer itself starts 4, 8 or 12 bytes past a 16-byte boundary (a slice of a caller's tensor)."""
    stream = torch.cuda.Stream()
    n, width = 5, 1001
    rows = TC.rows_of("softmax", n, width, 1, seed=shift)
    rows[1] = TC.rows_of("special", 1, width, 1)[0]
    flat = np.concatenate([np.zeros(shift, np.float32), rows.ravel(), np.zeros(4, np.float32)])
    d_all = torch.from_numpy(flat.view(np.int32).copy()).cuda()
    assert d_all.data_ptr() % 16 == 0
    for mk in ("interleaved", "sizes", "quarter_out"):
        co, C = PC.map_of(mk, width)
        pool = api.ClassPool(co, C)
        d_out = torch.empty(n * C + PAD + shift, dtype=torch.float32, device="cuda")[shift:]  # the output off alignment as well
        want = api.pool_ref(rows, co, C)
        for got in run_modes(torch, stream, pool, d_all.data_ptr() + 4 * shift, n, d_out):
            assert PC.same_bytes(got, want), (mk, shift)
        pool.delete()
    assert np.array_equal(d_all.cpu().numpy().view(np.uint32), flat.view(np.uint32))


@pytest.mark.parametrize("width,mk", [(251, "interleaved"), (8000, "sizes"), (RW + 1, "blocks"), (65, "none")])
def test_guarded_buffers(torch, width, mk):
    """Every element of the output is written, nothing around it is, and the input allocation keeps its bytes, with poison
    (NaN) around the rows that no result may meet."""
    n = 7
    rows = TC.rows_of("softmax", n, width, 1, seed=3)
    co, C = PC.map_of(mk, width)
    pool = api.ClassPool(co, C)
    want = api.pool_ref(rows, co, C)
    head, tail = in_guard(width)
    for mode in (0, 1, 2):
        api.set_pool_kernel(mode)
        g_in = guarded(torch.from_numpy(rows).cuda(), torch.float32, head, min(tail, 4 * width), byte_offset=4, fill=float("nan"), name="d_rows")
        g_out = guarded(n * C, torch.float32, out_guard(C) // 64, out_guard(C) // 64, byte_offset=12, device="cuda", name="d_out")
        pool.rows_device(g_in.ptr, n, g_out.ptr)
        torch.cuda.synchronize()
        g_in.check(f"mode {mode}")
        g_out.check(f"mode {mode}")
        assert PC.same_bytes(g_out.view.cpu().numpy().reshape(n, C), want), mode
    api.set_pool_kernel(0)
    pool.delete()


def test_composition_with_the_topk_selection(torch):
    """fdnn_topk_rows_device on the pooled rows: the k best CLASSES of every frame, equal to the numpy selection of them."""
    n, width, k = 33, 8000, 5
    rows = TC.rows_of("softmax", n, width, 1, seed=9)
    co, C = PC.map_of("interleaved", width)
    pool = api.ClassPool(co, C)
    d_rows = torch.from_numpy(rows).cuda()
    d_q = torch.empty(n * C, dtype=torch.float32, device="cuda")
    d_nodes = torch.empty(n * k, dtype=torch.int32, device="cuda")
    d_vals = torch.empty(n * k, dtype=torch.float32, device="cuda")
    pool.rows_device(d_rows.data_ptr(), n, d_q.data_ptr())
    api.topk_rows_device(d_q.data_ptr(), n, C, k, d_nodes.data_ptr(), d_vals.data_ptr())
    torch.cuda.synchronize()
    want = TC.select(api.pool_ref(rows, co, C), k)
    assert np.array_equal(d_nodes.cpu().numpy().reshape(n, k), want[0])
    assert np.array_equal(d_vals.cpu().numpy().view(np.uint32).reshape(n, k), want[1])
    pool.delete()


def test_argument_errors_launch_nothing(torch):
    for co, C in (([0, 1, -2], 2), ([0, 2, 1], 2), ([0, 0, 0], 4), ([0, 0, 0], 0)):
        with pytest.raises(api.FdnnError):
            api.ClassPool(np.array(co, np.int32), C)
    pool = api.ClassPool(np.arange(100, dtype=np.int32) % 3, 3)
    d = torch.zeros(4 * 100, dtype=torch.float32, device="cuda")
    dq = torch.full((4 * 3,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    before = api.pool_launches()
    for n, rows_ptr, out_ptr in ((-1, d.data_ptr(), dq.data_ptr()), (4, 0, dq.data_ptr()), (4, d.data_ptr(), 0)):
        with pytest.raises(api.FdnnError) as e:
            pool.rows_device(rows_ptr, n, out_ptr)
        assert e.value.code == api.FDNN_E_ARG, n
    pool.rows_device(d.data_ptr(), 0, dq.data_ptr())  # n == 0: a no-op
    torch.cuda.synchronize()
    assert api.pool_launches() == before and (dq == -7.0).all()
    pool.delete()
