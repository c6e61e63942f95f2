"""The large-batch rule of the half net without a device (csrc/fdnn_half.hpp: large_applies, gemm_grid)."""
import pytest

from fast_dnn_amd import api


def test_symbols():
    assert all(hasattr(api.lib(), name) for name in ("fdnn_half_model_set_large", "fdnn_debug_half_large_launches", "fdnn_debug_half_large_plan"))
    assert set(api.half_large_launches()) == {"large.sigmoid", "large.exp", "large.sigmoid.tap", "large.exp.tap"}


@pytest.mark.parametrize("small,mid,large", [(0, 0, 0), (0, 0, 1), (128, 4096, 1), (0, 200, 250), (128, 1000, 1001), (32, 0, 4097), (0, 4097, 3000)])
def test_rule(small, mid, large):
    """A call is large for n >= large >= 1 unless it is small (1 <= n <= small <= 128) or mid (1 <= n <= mid <= 4096 and not
    small); frame tiles of 256."""
    for n in range(4201):
        is_small = 1 <= n <= small <= 128
        is_mid = 1 <= n <= mid <= 4096 and not is_small
        is_large = large >= 1 and n >= large and not is_small and not is_mid
        assert api.half_large_plan(n, small, mid, large, 256, 0) == ((True, (n + 255) // 256, 2) if is_large else (False, 0, 0)), n


@pytest.mark.parametrize("rows_pad", [256, 2048, 8192])
def test_grid_and_refusals(rows_pad):
    """(ceil(n / 256), rows_pad / 128) in both forms: the tiled kernel's grid.  Bad rows_pad / act values are refused."""
    for n in (1, 257, 4096, 10000):
        assert all(api.half_large_plan(n, 0, 0, 1, rows_pad, act) == (True, -(-n // 256), rows_pad // 128) for act in (0, 1))
    for bad_rows, act in ((0, 0), (100, 0), (rows_pad - 64, 1), (rows_pad, 2)):
        with pytest.raises(api.FdnnError):
            api.half_large_plan(300, 0, 0, 1, bad_rows, act)
