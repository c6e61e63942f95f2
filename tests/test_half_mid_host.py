"""The mid-batch rule of the half net without a device (csrc/fdnn_half.hpp: mid_applies, mid_grid)."""
import pytest

from fast_dnn_amd import api


def test_symbols():
    for name in ("fdnn_half_model_set_mid", "fdnn_debug_half_mid_launches", "fdnn_debug_half_mid_plan"):
        assert hasattr(api.lib(), name), name


@pytest.mark.parametrize("small,mid", [(0, 0), (0, 4096), (128, 4096), (128, 100), (32, 1000), (0, 4097)])
def test_rule(small, mid):
    """A call is mid for 1 <= n <= mid <= 4096 unless it is small (1 <= n <= small <= 128); frame tiles of 64."""
    for n in range(4101):
        is_small = 1 <= n <= small <= 128
        is_mid = 1 <= n <= mid <= 4096 and not is_small
        assert api.half_mid_plan(n, small, mid, 256, 0) == ((True, (n + 63) // 64, 4) if is_mid else (False, 0, 0)), n


@pytest.mark.parametrize("rows_pad", [128, 256, 8064])
def test_grid(rows_pad):
    """(ceil(n / 64), rows_pad / 64) in both forms: a workgroup owns 64 nodes, one partial of the output form."""
    for n in (129, 1000, 4096):
        for act in (0, 1):
            assert api.half_mid_plan(n, 128, 4096, rows_pad, act) == (True, -(-n // 64), rows_pad // 64)


def test_refusals():
    for rows_pad, act in ((0, 0), (100, 0), (256, 2)):
        with pytest.raises(api.FdnnError):
            api.half_mid_plan(129, 128, 4096, rows_pad, act)
