"""Splicing raw feature frames, host side (convert.splice_frames / load_splice_offsets) and the C-ABI of the raw entry
points.  CPU only.

The reference's own data shows what splicing is: every 429-wide row of data/16khz and data/8khz is 11 x 39 values, row t
holding raw frames t-5 .. t+5, the first row repeating frame 0 for its left context."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np

from conftest import GOLDEN, ROOT, golden
from fast_dnn_amd import api
from fast_dnn_amd import convert as CV

NEW_ENTRY_POINTS = [
    "fdnn_model_set_splice", "fdnn_model_get_splice", "fdnn_calculate_raw", "fdnn_calculate_raw_device",
    "fdnn_calculate_lazy_bits_raw", "fdnn_ctx_forward_hidden_raw", "fdnn_stream_create", "fdnn_stream_free",
    "fdnn_stream_reset", "fdnn_stream_position", "fdnn_stream_push", "fdnn_stream_ctx", "fdnn_server_submit_raw",
]


def reference_rows_and_raw(name, tmp_path):
    """(the shipped 429-wide rows, the raw 39-wide frames they were spliced from)"""
    p = tmp_path / name
    p.write_bytes(golden("feat_files.npz")[name].tobytes())
    (_, rows), = CV.load_feature_text(str(p))
    # raw frame t = block 5 of row t; the last five frames = blocks 6 .. 10 of the last row
    raw = np.concatenate([rows[:, 5 * 39:6 * 39], rows[-1, 6 * 39:].reshape(5, 39)])
    return rows, np.ascontiguousarray(raw)


def test_reference_data_is_the_splice_of_its_raw_frames(tmp_path):
    for name, n_rows in (("16khz", 193), ("8khz", 389)):
        rows, raw = reference_rows_and_raw(name, tmp_path)
        assert rows.shape == (n_rows, 429) and raw.shape == (n_rows + 5, 39)
        got = CV.splice_frames(raw, range(-5, 6), 429, stream=True)
        assert got.shape == rows.shape
        assert got.tobytes() == rows.tobytes()  # byte for byte
    # padded to the net's 432, the first 100 rows are the reference's own 16khz.bin, three zero columns included
    _, raw16 = reference_rows_and_raw("16khz", tmp_path)
    b = golden("feat_files.npz")["16khz_bin"].tobytes()
    n_header, dim = struct.unpack(">ii", b[:8])
    want = np.frombuffer(b[8:], dtype=">f4").reshape(-1, dim)[:n_header].astype(np.float32)
    got = CV.splice_frames(raw16, range(-5, 6), 432)[:100]
    assert n_header == 100 and dim == 432
    assert got.tobytes() == want.tobytes()
    assert (got[:, 429:] == 0).all()
    assert got.tobytes() == golden("tiny.npz")["x16"].tobytes()  # the rows the golden oracle vectors were computed on


def test_splice_frames_definition():
    raw = np.arange(5 * 3, dtype=np.float32).reshape(5, 3)
    # clamped at both ends for a whole utterance; zero padding up to the width
    got = CV.splice_frames(raw, [-1, 0, 2], 12)
    want = np.zeros((5, 12), np.float32)
    for t in range(5):
        for j, o in enumerate([-1, 0, 2]):
            want[t, 3 * j:3 * j + 3] = raw[min(max(t + o, 0), 4)]
    assert np.array_equal(got, want)
    # stream: only rows whose right context has arrived; a left-only spec emits every frame
    assert np.array_equal(CV.splice_frames(raw, [-1, 0, 2], 12, stream=True), want[:3])
    assert CV.splice_frames(raw, [-2, -1, 0], 9, stream=True).shape == (5, 9)
    # identity, duplicates, any order
    assert np.array_equal(CV.splice_frames(raw, [0], 3), raw)
    dup = CV.splice_frames(raw, [1, 1, -3], 9)
    assert np.array_equal(dup[:, 0:3], dup[:, 3:6]) and np.array_equal(dup[:, 6:9], raw[[0, 0, 0, 0, 1]])
    assert CV.splice_frames(raw[:0], [-5, 5], 6).shape == (0, 6)
    for bad in ([], list(range(5))):
        try:
            CV.splice_frames(raw, bad, 12)
        except ValueError:
            continue
        raise AssertionError(f"offsets {bad} accepted")


def test_load_splice_offsets(tmp_path):
    # the toy fixture's header says "<Splice> 3 3": the offsets come from the bracket
    assert CV.load_splice_offsets(os.path.join(GOLDEN, "kaldi_toy", "final.feature_transform.txt")) == list(range(-5, 6))
    p = tmp_path / "no_splice.txt"
    p.write_text("<Nnet>\n<AddShift> 3 3\n<LearnRateCoef> 0 [ 0.9 1 0.007 ]\n<Rescale> 3 3\n"
                 "<LearnRateCoef> 0 [ -0.004 0.0625 0.015625 ]\n</Nnet>\n", encoding="utf-8")
    assert CV.load_splice_offsets(str(p)) is None
    q = tmp_path / "odd.txt"
    q.write_text("<Nnet>\n<Splice> 117 39\n[ 0 -2 2 2 ]\n<AddShift> 3 3\n[ 1 2 3 ]\n</Nnet>\n", encoding="utf-8")
    assert CV.load_splice_offsets(str(q)) == [0, -2, 2, 2]
    # the converter itself still drops the block, as the reference does
    shift, scale = CV.load_feature_transform_text(os.path.join(GOLDEN, "kaldi_toy", "final.feature_transform.txt"))
    assert shift.size == 3 and scale.size == 3


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(fdnn_[a-z0-9_]+)\s*\(", txt))


def test_raw_entry_points_are_declared_and_exported():
    decl = _declared("fdnn.h")
    L = api.lib()
    nm = shutil.which("nm")
    exported = None
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW_ENTRY_POINTS:
        assert name in decl, f"{name} is not declared in include/fdnn.h"
        assert name in api.SIGNATURES, f"{name} has no Python binding"
        assert hasattr(L, name)
        if exported is not None:
            assert name in exported, f"{name} is not exported by {api.LIB_PATH}"

