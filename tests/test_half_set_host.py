"""The half net's set step without a device (csrc/fdnn_half_set.hpp: applies, plan)."""
import os

import pytest

from conftest import ROOT
from fast_dnn_amd import api

NAMES = ("fdnn_half_calculate_lazy_sets", "fdnn_half_calculate_lazy_set", "fdnn_half_calculate_lazy_sets_device", "fdnn_debug_half_set_layer", "fdnn_debug_half_set_layer_us",
         "fdnn_debug_half_set_launches", "fdnn_debug_half_set_plan")


def test_symbols():
    header = open(os.path.join(ROOT, "include", "fdnn.h")).read()
    for name in NAMES:
        assert name in api.SIGNATURES and hasattr(api.lib(), name) and "FDNN_API int " + name + "(" in header, name
    for name in ("calculateLazySets", "calculateLazySet", "calculateLazySetsDevice", "setLayer"):
        assert callable(getattr(api.HalfDnn, name)), name
    assert set(api.half_set_launches()) == {"set.score", "set.score.tap", "set.gather"}


@pytest.mark.parametrize("K_pad,applies", [(32, True), (2048, True), (2080, False)])
def test_applies(K_pad, applies):
    assert api.half_set_plan([0, 10], [0, 3], K_pad)[0] is applies


def test_plan_literal_table():
    """Rows 0 5 5 40 70 129 with sets of 3, 0, 0, 40 and 131 nodes: segments 1 (no rows) and 2 (no nodes) have no workgroups;
    the others have 1, 2 and 5 node tiles of 32 and, at up to four frame tiles a workgroup, one frame group each."""
    assert api.half_set_plan([0, 5, 5, 40, 70, 129], [0, 3, 3, 3, 43, 174], 64, 192) == (True, 1, 1 + 0 + 2 + 5, 2)
    assert api.half_set_plan([0, 0], [0, 7], 64) == (True, 0, 0, 0)


@pytest.mark.parametrize("n_segs,launches", [(64, 1), (65, 2), (130, 3)])
def test_launches_hold_at_most_64_segments(n_segs, launches):
    """100-frame segments of 80 nodes: three node tiles each, four frame tiles to a workgroup."""
    rows = [100 * s for s in range(n_segs + 1)]
    ptr = [80 * s for s in range(n_segs + 1)]
    assert api.half_set_plan(rows, ptr, 2048) == (True, launches, 3 * n_segs, 4)


def test_a_long_segment_is_grouped_to_the_device():
    """One 80-node set over 10 000 frames: 313 frame tiles; the smallest group with which 3 node tiles x groups <= 256."""
    applies, launches, blocks, tpg = api.half_set_plan([0, 10000], [0, 80], 2048, n_cu=256)
    assert (applies, launches) == (True, 1) and blocks == 3 * -(-313 // tpg) <= 256 < 3 * -(-313 // (tpg - 1))


def test_refusals():
    for rows, ptr in (([0, 5, 3], [0, 1, 2]), ([0, 5], [1, 2]), ([0, 5], [0, -1])):
        with pytest.raises(api.FdnnError):
            api.half_set_plan(rows, ptr, 2048)
