"""The splice kernel that reads its segment table from device memory (fdnn_splice.hip, splice_table_kernel; the scoring loop's
live batches take it), alone: host in, host out through ``api.splice_table``.  Compared with the numpy definition --
row t of segment (row, center, lo, hi) is raw[clip(center + (t - row) + o, lo, hi)] per offset o, then zeros -- and with the
by-value kernel's launches on the same table.  The rows are copies: every comparison is np.array_equal."""
import numpy as np
import pytest

from fast_dnn_amd import api

pytestmark = pytest.mark.gpu

WIDTH = 432
SPECS = {"kaldi11": (list(range(-5, 6)), 39), "three144": ([-2, 0, 3], 144), "identity": ([0], 432),
         "left_only": (list(range(-10, 1)), 39), "duplicates": ([2, -1, 2, 0, -1, 5], 64)}
# segment tables: (segments, rows per segment lo .. hi)
TABLES = {"one": (1, 200, 200),          # one segment
          "s97": (97, 1, 5),             # the first count the by-value kernel cannot take in one launch
          "s1000x1": (1000, 1, 1),       # one row each
          "s300": (300, 1, 40)}          # 256 lanes cover 2.4 rows of 432: boundaries fall inside a workgroup's range (and 4 096 rows at most)


def make_table(spec, n_segs, lo_rows, hi_rows, rng):
    """Segments laid over ONE raw buffer as utterances are: each owns frames [lo, hi] and its rows' centres run inside them, so
    the clamps bite at both ends wherever a centre is within L of lo or within R of hi.  Every third segment has a single raw
    frame (lo == hi); every fifth starts at its own first frame and every seventh ends at its own last."""
    L, R = max(0, -min(spec[0])), max(0, max(spec[0]))
    segs, row, frame = [], 0, 0
    budget = 4096
    for g in range(n_segs):
        # (wide ranges: mostly short segments, every fourth from the whole range, so that 300 segments stay within 4 096 rows)
        rows = int(rng.integers(lo_rows, (hi_rows if hi_rows <= 5 or g % 4 == 0 else 5) + 1))
        rows = max(1, min(rows, budget - (n_segs - g - 1) - row))
        if g % 3 == 2:
            lo = hi = frame
            center = lo - int(rng.integers(0, 3))  # the rows' centres run across the one frame and beyond it
        else:
            before, after = (0 if g % 5 == 0 else int(rng.integers(0, L + 2))), (0 if g % 7 == 0 else int(rng.integers(0, R + 2)))
            lo, center = frame, frame + before
            hi = center + rows - 1 + after
        segs.append((row, center, lo, hi))
        row += rows
        frame = hi + 1
    return np.array(segs, dtype=np.int32), row, frame


def definition(spec, raw, segs, rows):
    offsets, D = spec
    x = np.zeros((rows, WIDTH), dtype=np.float32)
    ends = list(segs[1:, 0]) + [rows]
    for (row, center, lo, hi), end in zip(segs, ends):
        t = np.arange(row, end)
        for j, o in enumerate(offsets):
            x[row:end, j * D:(j + 1) * D] = raw[np.clip(center + (t - row) + o, lo, hi)]
    return x


@pytest.mark.parametrize("table", TABLES, ids=list(TABLES))
@pytest.mark.parametrize("spec", SPECS, ids=list(SPECS))
def test_table_kernel_equals_the_definition_and_the_by_value_launches(spec, table):
    sp = SPECS[spec]
    rng = np.random.default_rng(sorted(SPECS).index(spec) * 10 + sorted(TABLES).index(table))
    segs, rows, frames = make_table(sp, *TABLES[table], rng)
    assert len(segs) == TABLES[table][0] and rows <= 4096
    assert (segs[:, 2] == segs[:, 3]).any() or len(segs) == 1
    raw = rng.standard_normal((frames, sp[1])).astype(np.float32)
    want = definition(sp, raw, segs, rows)
    before = api.live_launches()
    got = api.splice_table(sp[0], sp[1], WIDTH, raw, segs, rows, True)
    after = api.live_launches()
    assert after["launches"] == before["launches"] + 1, "the table kernel is one launch whatever the table's length"
    assert after["max_segs"] >= len(segs)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    by_value = api.splice_table(sp[0], sp[1], WIDTH, raw, segs, rows, False)
    assert api.live_launches() == after, "use_table = 0 must not reach the table kernel"
    assert np.array_equal(by_value.view(np.uint32), got.view(np.uint32))


def test_segments_that_reach_beyond_the_buffer_read_inside_it():
    """lo below 0 and hi past the last frame: the frames read are never outside [max(lo, 0), min(hi, frames - 1)], for both
    kernels."""
    sp = SPECS["kaldi11"]
    raw = np.random.default_rng(5).standard_normal((12, 39)).astype(np.float32)
    segs = np.array([(0, 0, -4, 5), (6, 6, 6, 40)], dtype=np.int32)
    clipped = segs.copy()
    clipped[:, 2] = np.maximum(segs[:, 2], 0)
    clipped[:, 3] = np.minimum(segs[:, 3], 11)
    want = definition(sp, raw, clipped, 12)
    for use_table in (True, False):
        assert np.array_equal(api.splice_table(sp[0], sp[1], WIDTH, raw, segs, 12, use_table), want)
