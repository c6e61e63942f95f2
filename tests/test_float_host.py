"""The unquantized net, the half that needs no GPU: the stand-alone checker of fdnn_float.hpp and the float loader under the
sanitizers, the host restatement of a layer's sums against float64 (float_ref, bound 1), the planted faults that bound and
byte comparison must reject, the declarations, and what the C-ABI answers without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import float_ref as FR
from conftest import ROOT
from fast_dnn_amd import api, formats as F

NAMES = ("fdnn_float_model_load", "fdnn_float_model_load_on", "fdnn_float_model_free", "fdnn_float_model_input_dim",
         "fdnn_float_model_output_dim", "fdnn_float_model_layer_count", "fdnn_float_model_layer_dim", "fdnn_float_model_device",
         "fdnn_float_calculate", "fdnn_float_calculate_device", "fdnn_debug_float_layer", "fdnn_debug_float_layer_us", "fdnn_debug_float_layer_ref",
         "fdnn_debug_float_input_ref", "fdnn_debug_float_set_chunk", "fdnn_debug_float_launches", "fdnn_report_create",
         "fdnn_report_free", "fdnn_report_reset", "fdnn_report_add_device", "fdnn_report_add", "fdnn_report_read")


def test_float_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "float_check")
    src = os.path.join(ROOT, "tests", "host", "float_check.cpp")
    inc = os.path.join(ROOT, "fast-dnn_amd", "csrc")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", inc, src, os.path.join(inc, "fdnn_model.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    scratch = tmp_path / "files"
    scratch.mkdir()
    run = subprocess.run([exe, str(scratch)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "float ok" in run.stdout


def test_float_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "fdnn.h")).read()
    for name in NAMES:
        assert name in api.SIGNATURES and hasattr(api.lib(), name) and name + "(" in header, name
    counts = api.float_launches()
    assert list(counts) == list(api.FLOAT_LAUNCH_KINDS) and len(counts) == 8
    assert not any(n.startswith(("fgemm", "float", "report")) for n in api.launch_names())  # counted apart from the recorder's table


def _layer_ref(w, b, x):
    return api.float_layer_ref(w, b, x)


CASES = {  # name -> (n, K, rows, scale of x)
    "K20": (5, 20, 48, 20.0),
    "K48": (7, 48, 131, 1.0),
    "K432": (4, 432, 64, 20.0),
    "K1": (3, 1, 4, 1.0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_is_within_the_bound_of_float64(name):
    n, K, rows, sx = CASES[name]
    rng = np.random.default_rng(K)
    x = (rng.standard_normal((n, K)) * sx).astype(np.float32)
    w = (rng.standard_normal((rows, K)) * 0.05).astype(np.float32)
    b = (rng.standard_normal(rows) * 0.1).astype(np.float32)
    z = _layer_ref(w, b, x)
    assert z.dtype == np.float32 and z.shape == (n, rows)
    assert not FR.lin_failures(z, x, w, b).any()
    for what, zf in FR.planted_faults(x, w, b, _layer_ref).items():
        assert not FR.same_bits(z, zf), f"{name}: '{what}' leaves the bytes unchanged"


def test_long_k_case_rejects_every_planted_fault_by_the_bound():
    x, w, b = FR.long_k_case()
    K = x.shape[1]
    assert K == 2064 and K % 32 == 16
    terms = np.abs(x[:, None, :].astype(np.float64) * w[None, :8, :].astype(np.float64))
    bound = FR.lin_bound(x, w, b)
    assert terms.min() >= 0.5625 - 1e-6 and bound.max() <= 0.255 < 0.5 * terms.min()  # the premise: t_min > 2 bound
    z = _layer_ref(w, b, x)
    assert not FR.lin_failures(z, x, w, b).any()
    faults = FR.planted_faults(x, w, b, _layer_ref)
    assert len(faults) == 5
    for what, zf in faults.items():
        bad = FR.lin_failures(zf, x, w, b)
        assert not FR.same_bits(z, zf), what
        if what == "the last K mod 32 terms skipped":  # 16 signed terms may cancel in an output: most, not all
            assert bad.mean() > 0.5, what
        else:
            assert bad.all(), f"'{what}' passes bound 1 in {int((~bad).sum())} outputs"


def test_input_step_restatement_rounds_twice():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((9, 20)) * 20).astype(np.float32)
    sh = (rng.standard_normal(20) * 0.1).astype(np.float32)
    sc = rng.uniform(0.05, 0.07, 20).astype(np.float32)
    lin, act = api.float_input_ref(sh, sc, x)
    t = (x + sh[None, :]).astype(np.float32)
    assert FR.same_bits(lin, t) and FR.same_bits(act, (t * sc[None, :]).astype(np.float32))


def test_sigmoid_bound_holds_for_an_emulated_sequence():
    """The device's sequence emulated with float64 exp2 rounded to fp32 and pushed one ulp either way: inside the bound."""
    z = np.concatenate([np.linspace(-100, 100, 20001), [-120.0, 120.0, 0.0, -89.0, 104.0]]).astype(np.float32)
    y = (z * np.float32(-1.44269504088896340736)).astype(np.float32)
    with np.errstate(over="ignore", under="ignore"):
        e0 = np.exp2(y.astype(np.float64)).astype(np.float32)
    ends = None
    for e in (e0, np.nextafter(e0, np.float32(np.inf)), np.nextafter(e0, np.float32(0))):
        e = np.where(e < np.float32(2.0 ** -126), np.float32(0), e).astype(np.float32)  # v_exp_f32 flushes
        with np.errstate(over="ignore"):
            d = (np.float32(1.0) + e).astype(np.float32)
            s = (np.float32(1.0) / d).astype(np.float32)
        assert not FR.sigmoid_failures(s, z).any()
        ends = s[-5:] if ends is None else ends
    assert ends[0] == 0.0 and ends[3] == 0.0 and ends[1] == 1.0 and ends[4] == 1.0 and ends[2] == 0.5  # z = -120, -89, 120, 104, 0


def test_float_model_has_no_cpu_path(tiny_model_path):
    if api.device_count() > 0:
        pytest.skip("a GPU is present")
    h = C.c_void_p()
    assert api.lib().fdnn_float_model_load(tiny_model_path.encode(), C.byref(h)) == api.FDNN_E_DEVICE
    assert "no CPU path" in api.lib().fdnn_last_error().decode()
    with pytest.raises(api.FdnnError) as e:
        api.FloatDnn.loadFromFile(tiny_model_path)
    assert e.value.code == api.FDNN_E_DEVICE
    with pytest.raises(api.FdnnError) as e:
        api.AccuracyReport(10)
    assert e.value.code == api.FDNN_E_DEVICE


def test_float_loader_rejects_through_the_c_abi(tmp_path):
    def code(path):
        h = C.c_void_p()
        return api.lib().fdnn_float_model_load(str(path).encode(), C.byref(h))

    assert code(tmp_path / "missing.bin") == api.FDNN_E_IO
    bad = {"three layers": [20, 16, 16, 5], "hidden width 24": [20, 24, 24, 24, 5], "unequal widths": [20, 16, 32, 32, 5]}
    for what, topo in bad.items():
        p = tmp_path / "bad.bin"
        F.write_model_bin(str(p), F.synth_net(topo, seed=2))
        assert code(p) == api.FDNN_E_FORMAT, what
        # the quantized loader says the same about the same file
        hq = C.c_void_p()
        assert api.lib().fdnn_host_model_load(str(p).encode(), 3.0, C.byref(hq)) == api.FDNN_E_FORMAT, what
    good = tmp_path / "good.bin"
    F.write_model_bin(str(good), F.synth_net([20, 16, 16, 16, 5], seed=2))
    data = good.read_bytes()
    (tmp_path / "trunc.bin").write_bytes(data[:-5])
    assert code(tmp_path / "trunc.bin") == api.FDNN_E_FORMAT
    assert "truncated" in api.lib().fdnn_last_error().decode()
    h = C.c_void_p()
    assert api.lib().fdnn_float_model_load(str(good).encode(), C.byref(h)) in (api.FDNN_OK, api.FDNN_E_DEVICE)  # a good file gets as far as the device
    api.lib().fdnn_float_model_free(h)
    assert api.lib().fdnn_float_model_load(None, C.byref(h)) == api.FDNN_E_ARG
    assert api.lib().fdnn_debug_float_layer_ref(None, None, 1, 1, None, 1, None) == api.FDNN_E_ARG


def test_accuracy_tool_refuses_a_feature_file_of_another_width(tmp_path, monkeypatch):
    """Before any device call: the device entry points take raw pointers and cannot check a row's width themselves."""
    import importlib.util
    import sys

    spec = importlib.util.spec_from_file_location("accuracy_report_tool", os.path.join(ROOT, "tools", "accuracy_report.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    model, feats = str(tmp_path / "m18.bin"), str(tmp_path / "f.bin")
    F.write_model_bin(model, F.synth_net([18, 16, 16, 16, 10], seed=31))
    for width in (17, 19, 21, 432):
        F.write_feature_bin(feats, np.zeros((3, width), np.float32))
        monkeypatch.setattr(sys, "argv", ["accuracy_report.py", model, feats])
        with pytest.raises(SystemExit) as e:
            tool.main()
        assert f"Input vector size {width} must be equal with network input size 20" in str(e.value), width
    x = np.arange(54, dtype=np.float32).reshape(3, 18)
    padded = tool.fit_width(x, 18, 20)
    assert padded.shape == (3, 20) and (padded[:, :18] == x).all() and (padded[:, 18:] == 0).all()
    assert tool.fit_width(padded, 18, 20) is not None and tool.fit_width(padded, 18, 20).shape == (3, 20)
