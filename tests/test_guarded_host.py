"""tests/guarded.py on CPU tensors: every fault the GPU tests rely on it to see is planted here and must be reported, and
the same fault moved just out of the helper's reach must not be -- the reach is the guard sizes, which come from the kernels
(the largest frame tile, 320 rows, of rows padded to the widest node tile, 256 nodes)."""
import numpy as np
import pytest
import torch

import guarded as G

N, W = 5, 251  # rows off the 16-byte grid, padded width 256


def _out(byte_offset=12, tail=None, dtype=torch.float32):
    g = G.guarded(N * W, dtype, G.out_guard(W), G.out_guard(W) if tail is None else tail, byte_offset, name="out")
    return g


def _written(g):
    """As a correct kernel leaves it: every element of the view written, nothing else."""
    g.view[:] = 0.25 if g.dtype == torch.float32 else 3
    return g


def test_guard_sizes_come_from_the_tiles():
    assert G.out_guard(251) == 320 * 256 and G.out_guard(256) == 320 * 256 and G.out_guard(257) == 320 * 512 and G.out_guard(8000) == 320 * 8192
    assert G.in_guard(432) == (432, 320 * 432)


@pytest.mark.parametrize("dtype,size,offsets", [(torch.float32, 4, (0, 4, 8, 12, 16)), (torch.int32, 4, (0, 4, 8, 12)), (torch.int8, 1, (0, 1, 3, 8, 15)),
                                                (torch.int64, 8, (0, 8))])
def test_view_is_the_payloads_extent_at_the_offset(dtype, size, offsets):
    for off in offsets:
        fill = {torch.int8: -128, torch.int64: -1}.get(dtype)
        g = G.guarded(N * W, dtype, 7, 9, off, fill=fill)
        assert g.view.numel() == N * W and g.view.dtype == dtype and g.view.is_contiguous()
        assert (g.ptr - off) % 256 == 0 and g.ptr == g.view.data_ptr()
        assert g.whole.numel() == 7 + N * W + 9 and g.whole[7:].data_ptr() == g.ptr
        assert g.ptr - 7 * size - g.raw.data_ptr() >= G.SLACK  # (never against the allocation's edge)
    with pytest.raises(ValueError):
        G.guarded(N * W, torch.float32, 7, 9, 6)


def test_sentinels_are_what_no_result_equals():
    g = _out()
    bits = g.whole.view(torch.int32)
    assert bool((bits == G.NAN_SENTINEL).all()) and bool(torch.isnan(g.whole).all())
    assert G.NAN_SENTINEL not in (0x7FC00000, np.int32(-0x400000))  # the NaNs arithmetic produces
    gi = _out(dtype=torch.int32)
    assert bool((gi.whole == G.INT_SENTINEL).all()) and G.INT_SENTINEL < 0


def test_a_clean_call_passes():
    _written(_out()).check()
    _written(_out(dtype=torch.int32)).check()


@pytest.mark.parametrize("where,label", [(-1, "before"), (N * W, "after"), (N * W + 319 * 256, "after"), (N * W + 320 * 256 - 1, "after"),
                                         (-320 * 256, "before")])
def test_a_write_outside_the_view_is_reported(where, label):
    g = _written(_out())
    g.whole[g.head + where] = 1.0
    with pytest.raises(AssertionError, match=f"write outside the buffer, {label} it, at element {where} "):
        g.check("case")


def test_a_write_of_the_sentinels_own_nan_class_is_reported():
    """A kernel that stores a NaN of its own outside the view: the guards are compared as bits, not as floats."""
    g = _written(_out())
    g.whole[g.head - 1] = float("nan")
    with pytest.raises(AssertionError, match="before it"):
        g.check()


def test_an_unwritten_element_is_reported():
    g = _written(_out())
    g.view.view(torch.int32)[N * W - 1] = G.NAN_SENTINEL  # the last element of the last row, as a tail loop one short leaves it
    with pytest.raises(AssertionError, match=f"1 elements of the buffer were never written, the first at {N * W - 1}"):
        g.check()
    gi = _out(dtype=torch.int32)
    gi.view[:] = 3
    gi.view[17] = G.INT_SENTINEL
    with pytest.raises(AssertionError, match="never written, the first at 17"):
        gi.check()


def _input(kind):
    rng = np.random.default_rng(3)
    if kind == "x":
        head, tail = G.in_guard(432)
        return G.guarded(rng.standard_normal((N, 432)).astype(np.float32), torch.float32, head, tail, 16, fill=float("nan"), name="x")
    if kind == "bytes":
        head, tail = G.in_guard(W)
        return G.guarded(rng.integers(-128, 128, (N, W)).astype(np.int8), torch.int8, head, tail, 3, fill=-128, name="masks")
    head, tail = G.in_guard(4)
    return G.guarded(rng.integers(0, 1 << 62, (N, 4)).astype(np.int64), torch.int64, head, tail, 8, fill=-1, name="bits")


@pytest.mark.parametrize("kind", ["x", "bytes", "bits"])
def test_inputs_are_poisoned_around_and_watched_as_a_whole(kind):
    g = _input(kind)
    assert g.is_input
    if kind == "x":
        assert bool(torch.isnan(g.whole[:g.head]).all()) and bool(torch.isnan(g.whole[g.head + g.count:]).all()) and not bool(torch.isnan(g.view).any())
    elif kind == "bytes":
        assert bool((g.whole[:g.head] == -128).all()) and bool((g.whole[g.head + g.count:] == -128).all())
    else:
        assert bool((g.whole[:g.head] == -1).all()) and bool((g.whole[g.head + g.count:] == -1).all())
    g.check()
    for at in (g.head, g.head + g.count - 1, 0, g.whole.numel() - 1):  # a modified input; modified poison is a stray write too
        keep = g.whole[at].clone()
        g.whole[at] = 1 if kind != "x" else 2.0
        with pytest.raises(AssertionError, match="the input allocation changed at byte"):
            g.check()
        g.whole[at] = keep
        g.check()


def test_a_refused_call_must_leave_the_output_untouched():
    g = _out()
    g.assert_untouched()
    g.view[N * W // 2] = 0.5
    with pytest.raises(AssertionError, match=f"written at element {N * W // 2} "):
        g.assert_untouched("refused")


# ---- the reach: the same faults just outside what the helper was asked to watch go unseen, so the sizes above are what finds them
def test_a_write_319_rows_out_needs_the_320_row_guard():
    short = _written(_out(tail=319 * 256))  # a guard of 319 padded rows: the store of row 319 of the last tile lands in the slack
    short.raw[short.whole.data_ptr() - short.raw.data_ptr() + 4 * (short.head + N * W + 319 * 256)] = 1
    short.check()
    full = _written(_out())
    full.raw[full.whole.data_ptr() - full.raw.data_ptr() + 4 * (full.head + N * W + 319 * 256)] = 1
    with pytest.raises(AssertionError, match="after it"):
        full.check()


def test_writes_past_either_guard_are_out_of_reach():
    g = _written(_out())
    first = g.whole.data_ptr() - g.raw.data_ptr()
    g.raw[first - 1] = 1                       # one byte before the head guard
    g.raw[first + 4 * g.whole.numel()] = 1     # one byte after the tail guard
    g.check()


def test_an_output_is_not_watched_for_content_and_an_input_is_not_asked_to_be_written():
    g = _written(_out())
    g.view[3] = 7.0  # any value but the sentinel is "written"
    g.check()
    _input("x").check()  # an input's interior holds no sentinel to look for
