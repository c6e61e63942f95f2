"""The half-precision net, the half that needs no GPU (csrc/fdnn_half.hpp): the declarations, the packed blob against
numpy's float16, the buffer extents of a call, and the premise of the long-k device test."""
import ctypes as C
import os

import numpy as np
import pytest

import half_ref as HR
from conftest import ROOT
from fast_dnn_amd import api, formats as F

NAMES = ("fdnn_half_model_load", "fdnn_half_model_load_on", "fdnn_half_model_free", "fdnn_half_model_input_dim", "fdnn_half_model_output_dim",
         "fdnn_half_model_layer_count", "fdnn_half_model_layer_dim", "fdnn_half_model_device", "fdnn_half_calculate",
         "fdnn_half_calculate_device", "fdnn_debug_half_layer", "fdnn_debug_half_layer_us", "fdnn_debug_half_set_chunk",
         "fdnn_debug_half_launches", "fdnn_debug_half_pack", "fdnn_debug_half_extents")


def test_half_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "fdnn.h")).read()
    for name in NAMES:
        assert name in api.SIGNATURES and hasattr(api.lib(), name) and name + "(" in header, name
    assert "fdnn_half.hpp" in header  # the contract is stated once, there
    assert list(api.half_launches()) == list(api.HALF_LAUNCH_KINDS) and len(api.HALF_LAUNCH_KINDS) == 5
    assert api.lib().fdnn_half_model_load(None, C.byref(C.c_void_p())) == api.FDNN_E_ARG


def test_pack_rounds_like_numpy_and_pads_by_the_contract(tmp_path):
    net = F.synth_net([18, 48, 48, 48, 131], seed=21, w0_std=0.05, w_std=0.3)
    rng = np.random.default_rng(9)
    w = net.layers[1].weights
    # ties between neighbouring halves (normal and subnormal), the subnormal range, the smallest and the largest that stay finite
    w[0, :8] = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(2 + 2.0 ** -10), 2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -14 - 2.0 ** -25), 65519.0, 2.0 ** -26]
    w[1:9] = (rng.uniform(-1, 1, (8, 48)) * 2.0 ** -14).astype(np.float32)
    w[9] = (rng.integers(-2047, 2048, 48) * 2.0 ** -25).astype(np.float32)  # every second one a subnormal tie
    path = str(tmp_path / "pack.bin")
    F.write_model_bin(path, net)
    pk = api.half_pack(path)
    blob, layers = pk["blob"], pk["layers"]
    assert [(l["rows"], l["rows_pad"], l["K"], l["K_pad"]) for l in layers] == [(48, 256, 20, 32), (48, 256, 48, 64), (48, 256, 48, 64), (131, 256, 48, 64)]
    for j, (l, spec) in enumerate(zip(layers, net.layers)):
        assert l["off_w"] % 256 == 0 and l["off_bias"] % 256 == 0 and l["off_bias"] + 4 * l["rows_pad"] <= blob.size
        W = blob[l["off_w"]:l["off_w"] + 2 * l["rows_pad"] * l["K_pad"]].view(np.uint16).reshape(l["rows_pad"], l["K_pad"])
        k_file = spec.weights.shape[1]  # layer 0: 18 in the file, padded to 20 with +0 weights, then to 32 with -0
        assert np.array_equal(W[:l["rows"], :k_file], spec.weights.astype(np.float16).view(np.uint16)), f"layer {j}: fp16 bytes"
        assert (W[:l["rows"], k_file:l["K"]] == 0).all() and (W[:l["rows"], l["K"]:] == 0x8000).all() and (W[l["rows"]:] == 0).all(), f"layer {j}: pads"
        bias = blob[l["off_bias"]:l["off_bias"] + 4 * l["rows_pad"]].view(np.float32)
        assert np.array_equal(bias[:l["rows"]], spec.bias) and (bias[l["rows"]:].view(np.uint32) == 0).all()
    sh = blob[pk["off_shift"]:pk["off_shift"] + 128].view(np.float32)
    sc = blob[pk["off_scale"]:pk["off_scale"] + 128].view(np.float32)
    assert pk["off_shift"] % 256 == 0 and pk["off_scale"] % 256 == 0 and pk["off_scale"] + 128 <= blob.size
    assert np.array_equal(sh[:18], net.shift) and np.array_equal(sc[:18], net.scale) and (sh[18:] == 0).all() and (sc[18:] == 0).all()
    net.layers[3].weights[130, 47] = 65520.0  # the tie between 65504 and 2^16: rounds to even, the infinite one
    F.write_model_bin(path, net)
    with pytest.raises(api.FdnnError) as e:
        api.half_pack(path)
    assert e.value.code == api.FDNN_E_FORMAT and "layer 3, node 130" in str(e.value)


@pytest.mark.parametrize("chunk", [100, 0])
def test_extents_of_every_call(chunk):
    """The tiny shape (k0_pad 32, act_ld 64, 131 of 256 output rows): every launch of every chunk stays inside what the call reserved."""
    for n in range(1, 601):
        e = api.half_extents((32, 64, 131, 256), n, chunk)
        cap = min(n, chunk or 4096)
        assert (e["xs"], e["act"], e["partial"]) == (cap * 32, cap * 64, cap * 4), n
        assert e["tiled"] == 1 and e["xs_touched"] <= e["xs"] and e["act_touched"] <= e["act"] and e["partial_touched"] <= e["partial"], n


def test_long_k_premise():
    x, w, b = HR.long_k_case()
    bound, t_min = HR.long_k_margin(x, w, b)
    assert x.shape == (129, 1040) and w.shape == (160, 1040) and 1040 % 32 == 16
    assert np.array_equal(x, HR.halves(x)) and np.array_equal(w, HR.halves(w))
    assert t_min >= 0.5625 and bound <= HR.gamma1(1041) * 1043 + 1e-30 and bound < 0.13 < 0.5 * t_min
    terms = x[:, None, :8].astype(np.float64) * w[None, :, :8]  # a single term is further from z64 than the bound allows
    assert np.abs(terms).min() > 2 * bound
