"""The quantization report on the device (fdnn_report_*, fdnn_float.hip) against a float64 numpy restatement of
FuncTest.diff: counts and the maximum are equal (integers, and a maximum has no order), sums are within 1e-12 relative
(n 2^-53 for n <= 9000 terms in double: the bound on ANY order of additions)."""
import contextlib
import importlib.util
import io
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from fast_dnn_amd import api, formats as F

pytestmark = pytest.mark.gpu

THR = 0.1
REL = 1e-12


def restate(ref, q, thr=THR):
    """FuncTest.diff in float64: rows with a NaN in either matrix are counted and left out."""
    nan = np.isnan(ref).any(axis=1) | np.isnan(q).any(axis=1)
    r, qq = ref[~nan], q[~nan]
    d = np.abs(qq.astype(np.float64) - r.astype(np.float64))
    node = d.sum(axis=0)
    return {"frames": ref.shape[0], "nan_rows": int(nan.sum()), "top1_agree": int((r.argmax(axis=1) == qq.argmax(axis=1)).sum()),
            "nodes_over": int((node > thr).sum()), "max_abs": float(d.max(initial=0.0)), "sum_abs": float(d.sum()), "node_sum": node,
            "max_node_sum": float(node.max(initial=0.0))}


def compare(rep, want, what):
    got = rep.read(THR, nodeSums=True)
    print(f"{what}: frames {got['frames']} nan_rows {got['nan_rows']} top1 {got['top1_agree_rows']} over {got['nodes_over_0.1']} "
          f"max_abs {got['max_abs_diff']:.9e} sum_abs {got['sum_abs_diff']:.15e} (numpy {want['sum_abs']:.15e})")
    assert got["frames"] == want["frames"] and got["nan_rows"] == want["nan_rows"], what
    assert got["top1_agree_rows"] == want["top1_agree"], what
    assert got["nodes_over_0.1"] == want["nodes_over"], what
    assert got["max_abs_diff"] == want["max_abs"], what
    assert abs(got["sum_abs_diff"] - want["sum_abs"]) <= REL * want["sum_abs"], what
    assert abs(got["max_node_sum_abs_diff"] - want["max_node_sum"]) <= REL * want["max_node_sum"], what
    assert (np.abs(got["node_sum"] - want["node_sum"]) <= REL * want["node_sum"]).all(), what
    used = want["frames"] - want["nan_rows"]
    if used:
        assert got["top1_agreement"] == want["top1_agree"] / used and got["nodes"] == want["node_sum"].size
        assert abs(got["mean_abs_diff"] - want["sum_abs"] / (used * got["nodes"])) <= REL * got["mean_abs_diff"] + 1e-300


def make(n, O, seed):
    """ref uniform in [0, 1); q = ref + noise of 1e-4 (node sums far below 0.1), every seventh node noise of 1e-2 (far above);
    two nodes whose sums sit 1e-6 above and below the threshold (one non-zero difference each: exact in any order);
    ties of the maximum in both matrices, with equal and with different first indices; one NaN row where there is room."""
    rng = np.random.default_rng(seed)
    ref = rng.random((n, O), dtype=np.float32)
    amp = np.where(np.arange(O) % 7 == 3, 1e-2, 1e-4).astype(np.float32)
    q = (ref + (rng.random((n, O), dtype=np.float32) - np.float32(0.5)) * amp[None, :]).astype(np.float32)
    a, b = 1, O - 1  # the straddling nodes
    q[:, a], q[:, b] = ref[:, a], ref[:, b]
    q[0, a] = np.float32(ref[0, a] + np.float32(THR + 1e-6))
    q[n - 1, b] = np.float32(ref[n - 1, b] + np.float32(THR - 1e-6))
    rows = list(range(n))
    if O >= 5:
        for i, (ra, rb, qa, qb) in zip(rows[0::3], [(0, 3, 0, 4), (2, 4, 3, 4), (1, 2, 1, 2)] * n):
            ref[i, [ra, rb]] = 2.0  # tie: the first index wins
            q[i, [qa, qb]] = 2.0
    if n >= 3:
        ref[n // 2, O // 2] = np.nan
    if n >= 200:
        q[n // 2 + 1, 0] = np.nan
        ref[n // 2 + 1, 1] = np.inf  # a NaN row's other values do not count
    return ref, q


@pytest.mark.parametrize("n,O", [(1, 5), (257, 131), (300, 8000)])
def test_report_equals_the_float64_restatement(n, O):
    import torch

    ref, q = make(n, O, seed=n + O)
    want = restate(ref, q)
    if n > 1:
        assert want["nan_rows"] >= 1 and 0 < want["top1_agree"] < want["frames"] - want["nan_rows"]
        assert 0 < want["nodes_over"] < O and want["node_sum"][1] > THR > want["node_sum"][O - 1] > THR - 2e-6
    before = api.float_launches()
    rep = api.AccuracyReport(O, device=0)
    try:
        rep.add(ref, q)
        compare(rep, want, f"host form ({n}, {O})")
        host = rep.read(THR, nodeSums=True)
        # two adds equal the restatement on the concatenation
        cut = n // 3
        rep.reset()
        assert rep.read(THR)["frames"] == 0 and rep.read(THR)["max_abs_diff"] == 0.0
        rep.add(ref[:cut], q[:cut])
        rep.add(ref[cut:], q[cut:])
        compare(rep, want, f"two adds ({n}, {O})")
        rep.add(ref, q)
        compare(rep, restate(np.concatenate((ref, ref)), np.concatenate((q, q))), f"accumulated ({n}, {O})")
        # the device form: the host form's figures, bit for bit
        rep.reset()
        rd, qd = torch.from_numpy(ref).cuda(), torch.from_numpy(q).cuda()
        torch.cuda.synchronize()
        rep.addDevice(rd.data_ptr(), qd.data_ptr(), n, 0)
        dev = rep.read(THR, nodeSums=True)
        assert np.array_equal(dev.pop("node_sum"), host.pop("node_sum")) and dev == host
    finally:
        rep.delete()
    after = api.float_launches()
    for kind in ("report.rows", "report.nodes", "report.fold"):
        assert after[kind] - before[kind] == (5 if cut else 4), kind  # one launch group per non-empty add


def test_report_over_more_rows_than_one_launch_group():
    """5000 rows: two launch groups (4096 + 904) reuse the row flags and the block partials; a NaN row in each."""
    import torch

    n, O = 5000, 5
    rng = np.random.default_rng(50)
    ref = rng.random((n, O), dtype=np.float32)
    q = (ref + (rng.random((n, O), dtype=np.float32) - np.float32(0.5)) * np.float32(1e-3)).astype(np.float32)
    q[::7, 2] = 2.0  # top-1 disagrees in every seventh row
    ref[10, 3] = np.nan
    q[4500, 0] = np.nan
    ref[4095, 4], ref[4096, 4] = 5.0, -5.0  # the rows either side of the group boundary carry the maximum
    want = restate(ref, q)
    assert want["nan_rows"] == 2 and 0 < want["top1_agree"] < n - 2
    before = api.float_launches()
    rep = api.AccuracyReport(O, device=0)
    try:
        rep.add(ref, q)
        compare(rep, want, "host form (5000, 5)")
        host = rep.read(THR, nodeSums=True)
        rep.reset()
        rd, qd = torch.from_numpy(ref).cuda(), torch.from_numpy(q).cuda()
        torch.cuda.synchronize()
        rep.addDevice(rd.data_ptr(), qd.data_ptr(), n, 0)
        dev = rep.read(THR, nodeSums=True)
        assert np.array_equal(dev.pop("node_sum"), host.pop("node_sum")) and dev == host
    finally:
        rep.delete()
    after = api.float_launches()
    assert after["report.nodes"] - before["report.nodes"] == 4  # two calls of two groups each


def _tool():
    spec = importlib.util.spec_from_file_location("accuracy_report_tool", os.path.join(ROOT, "tools", "accuracy_report.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_tool_pads_a_feature_file_of_the_models_own_width(tmp_path, monkeypatch):
    """A model whose stored input width (18) is no multiple of 4: the feature file has 18 columns, both nets read 20.  The
    tool's figures are those of the frames zero-padded by hand; a file of another width is refused before any device call."""
    net = F.synth_net([18, 16, 16, 16, 10], seed=31, w0_std=0.05, w_std=0.3)
    model, feats, wrong = str(tmp_path / "m18.bin"), str(tmp_path / "f18.bin"), str(tmp_path / "f17.bin")
    F.write_model_bin(model, net)
    x = F.synth_features(130, 18, seed=12, pad_from=None)
    F.write_feature_bin(feats, x)
    F.write_feature_bin(wrong, x[:, :17])
    tool = _tool()
    out = io.StringIO()
    monkeypatch.setattr(sys, "argv", ["accuracy_report.py", model, feats, "--cutoffs", "3"])
    with contextlib.redirect_stdout(out):
        tool.main()
    got = json.loads(out.getvalue().strip().splitlines()[-1])
    xp = np.concatenate((x, np.zeros((130, 2), np.float32)), axis=1)
    fdnn, qdnn = api.FloatDnn.loadFromFile(model, device=0), api.QuantizedDnn.loadFromFile(model, device=0)
    try:
        assert fdnn.inputDimension() == 20
        want = restate(fdnn.calculate(xp), qdnn.calculate(xp))
    finally:
        fdnn.delete()
        qdnn.delete()
    assert got["path"] == "device" and got["frames"] == 130 and got["nan_rows"] == 0
    assert got["max_abs_diff"] == want["max_abs"] and got["top1_agree_rows"] == want["top1_agree"]
    assert abs(got["sum_abs_diff"] - want["sum_abs"]) <= REL * want["sum_abs"]
    monkeypatch.setattr(sys, "argv", ["accuracy_report.py", model, wrong])
    with pytest.raises(SystemExit) as e:
        tool.main()
    assert "Input vector size 17 must be equal with network input size 20" in str(e.value)


def test_report_through_the_tools_path(tiny_model_path):
    """The float model and the quantized scorer on the same file and frames, both fed to the report."""
    fdnn = api.FloatDnn.loadFromFile(tiny_model_path, device=0)
    qdnn = api.QuantizedDnn.loadFromFile(tiny_model_path, device=0)
    rep = None
    try:
        assert fdnn.inputDimension() == qdnn.inputDimension() and fdnn.outputDimension() == qdnn.outputDimension()
        x = F.synth_features(257, fdnn.inputDimension(), seed=9, pad_from=None)
        ref, q = fdnn.calculate(x), qdnn.calculate(x)
        rep = api.AccuracyReport(fdnn.outputDimension(), device=0)
        rep.add(ref[:100], q[:100])
        rep.add(ref[100:], q[100:])
        compare(rep, restate(ref, q), "tiny model, float against quantized")
        assert np.isfinite(ref).all() and np.abs(ref.sum(axis=1) - 1.0).max() < 1e-4
    finally:
        if rep is not None:
            rep.delete()
        fdnn.delete()
        qdnn.delete()


def test_report_argument_errors():
    with pytest.raises(api.FdnnError) as e:
        api.AccuracyReport(0)
    assert e.value.code == api.FDNN_E_ARG
    rep = api.AccuracyReport(5)
    try:
        with pytest.raises(ValueError):
            rep.add(np.zeros((2, 4), np.float32), np.zeros((2, 4), np.float32))
        assert api.lib().fdnn_report_add(rep.h, None, None, 1) == api.FDNN_E_ARG
        assert api.lib().fdnn_report_read(rep.h, 0.1, None, None) == api.FDNN_E_ARG
        rep.add(np.zeros((0, 5), np.float32), np.zeros((0, 5), np.float32))  # n == 0: a no-op
        assert rep.read()["frames"] == 0
    finally:
        rep.delete()
