"""The small-batch rule of the half net without a device (csrc/fdnn_half.hpp: small_applies, small_grid)."""
import pytest

from fast_dnn_amd import api


def test_symbols():
    for name in ("fdnn_half_model_set_small", "fdnn_debug_half_small_launches", "fdnn_debug_half_small_plan"):
        assert hasattr(api.lib(), name), name


@pytest.mark.parametrize("setting", [0, 1, 32, 128])
def test_rule(setting):
    """A call is small for 1 <= n <= setting; its frame tiles are ceil(n / 32); the grid does not depend on n."""
    for n in range(131):
        applies, grid, tiles = api.half_small_plan(n, setting, 256, 0)
        assert (applies, grid, tiles) == ((True, 8, (n + 31) // 32) if 1 <= n <= setting else (False, 0, 0)), n


@pytest.mark.parametrize("rows_pad", [128, 256, 8064])
def test_grid(rows_pad):
    """One workgroup per node tile: 32 nodes in the hidden form, a whole 64-node partial in the output form."""
    assert api.half_small_plan(100, 128, rows_pad, 0) == (True, rows_pad // 32, 4)
    assert api.half_small_plan(100, 128, rows_pad, 1) == (True, rows_pad // 64, 4)


def test_refusals():
    assert api.half_small_plan(1, 129, 256, 0) == (False, 0, 0)  # no setting above 128 makes a call small
    for n, setting, rows_pad, act in ((1, 1, 0, 0), (1, 1, 100, 0), (1, 1, 256, 2)):
        with pytest.raises(api.FdnnError):
            api.half_small_plan(n, setting, rows_pad, act)
