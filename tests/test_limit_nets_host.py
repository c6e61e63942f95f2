"""The conditions of tests/limit_nets.py's builders, asserted with the CPU oracle alone, and the loader's limits through the
host half (api.HostModel).  No GPU: tests/test_gpu_model_limits.py compares the kernels with the oracle on these nets, and a
comparison on a net that forgot its input, or whose planted values are not where the builder says, would prove nothing."""
import os

import numpy as np
import pytest

import limit_nets as LN
import softmax_ref as SR
from fast_dnn_amd import api, formats as F
from oracle.oracle import Oracle

DEPTHS = LN.DEPTHS


def deep_file(tmp_models, n_hid, w_std, width=256):
    return LN.cached(tmp_models, f"limit_deep_{n_hid}x{width}", LN.deep_topology(n_hid, width), lambda: LN.deep_net(n_hid, width, w_std=w_std))


@pytest.mark.parametrize("n_hid,w_std", DEPTHS)
def test_deep_net_keeps_its_signal(tmp_models, n_hid, w_std):
    orc = Oracle(deep_file(tmp_models, n_hid, w_std))
    assert orc.n_layers == n_hid + 2
    x = F.synth_features(64, 432, seed=11)
    want, wt = orc.calculate(x, taps=True)
    frames, med, values = LN.assert_keeps_signal(wt["u8_acts"][-1], f"deep_net({n_hid})")
    assert not np.isnan(want).any() and len(np.unique(want, axis=0)) == 64
    assert wt["sat_events"] > (1000 if w_std == 0.5 else 0) or n_hid == 2  # (the walk runs at depth; two layers of the 0.3 net fire nothing)
    print(f"deep_net({n_hid}, w_std={w_std}): {frames} distinct frames, median range {med}, {values} byte values, {wt['sat_events']} events")
    orc.close()


def test_the_default_gaussian_net_would_fail_the_condition(tmp_models):
    """What the condition is for: the plain synth_net at depth 29 has lost its input (8 distinct frames of 64, range 0)."""
    topo = LN.deep_topology(29)
    orc = Oracle(LN.cached(tmp_models, "limit_gauss_29x256", topo, lambda: F.synth_net(topo, seed=7)))
    _, wt = orc.calculate(F.synth_features(64, 432, seed=11), taps=True)
    with pytest.raises(AssertionError):
        LN.assert_keeps_signal(wt["u8_acts"][-1], "synth_net at depth 29")
    orc.close()


def test_deep_net_at_production_width_keeps_its_signal(tmp_models):
    """[432] + [2048] * 10 + [252]: the 8 + 1 split of the chained launch on the kernel's own K."""
    orc = Oracle(LN.cached(tmp_models, "limit_deep_9x2048", LN.deep_topology(9, 2048), lambda: LN.deep_net(9, 2048)))
    hid = orc.hidden_acts_mt(F.synth_features(32, 432, seed=11))
    LN.assert_keeps_signal(hid, "deep_net(9, 2048)")
    orc.close()


@pytest.mark.parametrize("W", (65536, 65537, 131075, 524288))
def test_wide_out_net_has_no_probability_below_the_normals(tmp_models, W):
    orc = Oracle(LN.cached(tmp_models, f"limit_wide_out_{W}", LN.wide_out_topology(W), lambda: LN.wide_out_net(W)))
    x = F.synth_features(5, 432, seed=W % 977)
    _, wt = orc.calculate(x, taps=True)
    p64 = SR.softmax64(wt["logits"])
    assert p64.min() >= SR.TINY, p64.min()
    assert len(np.unique(wt["acc_out"], axis=0)) > 1  # (16 hidden nodes carry little: frames differ in few accumulators, but they differ)
    nodes = LN.edge_nodes(W)
    assert nodes.size == 80 and nodes[0] == 0 and nodes[-1] == W - 1 and all(v in nodes for m in range(65536, W + 1, 65536) for v in (m - 1, min(m, W - 1)))
    orc.close()


def test_extreme_acc_net_plants_what_it_says(tmp_models):
    path, info = LN.extreme_acc_file(tmp_models)
    orc = Oracle(path)
    x = F.synth_features(3, 432, seed=4)
    _, wt = orc.calculate(x, taps=True)
    LN.assert_planted(info, wt, orc)
    assert np.abs(info["acc"]).min() > (1 << 26) and np.abs(info["acc"]).max() == (LN.ACC_H // 2) * 32768
    assert info["hit"].sum() >= 10, info["hit"]
    # the planted rows' bytes are the table's at the solved pre-activations, and a quotient one ulp off changes most of them
    lin = LN.hidden_lin(info["acc"], info["coef"], info["bias"])
    assert np.array_equal(lin, info["lin"])
    assert np.array_equal(wt["u8_acts"][2][0, :LN.ACC_ROWS], np.array([Oracle.sigmoid_q(float(v)) for v in lin], np.uint8))
    either = info["sensitive_in"] | info["sensitive_out"]
    assert either.sum() >= 10 and info["sensitive_in"].sum() >= 4 and info["sensitive_out"].sum() >= 4, (info["sensitive_in"], info["sensitive_out"])
    assert np.abs(lin).max() < 1.5  # the steep part of the table
    orc.close()


# -------------------------------------------------------------------------------------------------------- loader limits
def _refused(path):
    with pytest.raises(api.FdnnError) as e:
        api.HostModel(path)
    return e.value


def test_loader_takes_31_affine_layers_and_refuses_32(tmp_models):
    topo = [432] + [16] * 30 + [8]
    p = LN.cached(tmp_models, "limit_affine_31", topo, lambda: F.synth_net(topo, seed=2))
    hm = api.HostModel(p)
    assert hm.n_layers == 31 and api.host_blob_check(hm.blob())["n_affine"] == 31
    hm.close()
    topo = [432] + [16] * 31 + [8]
    err = _refused(LN.cached(tmp_models, "limit_affine_32", topo, lambda: F.synth_net(topo, seed=2)))
    assert err.code == api.FDNN_E_FORMAT and "32 affine layers" in str(err) and "4..31" in str(err), str(err)


def test_loader_takes_2_19_outputs_and_refuses_one_more(tmp_models):
    W = 1 << 19
    hm = api.HostModel(LN.cached(tmp_models, f"limit_wide_out_{W}", LN.wide_out_topology(W), lambda: LN.wide_out_net(W)))
    assert hm.layer_out(hm.n_layers - 1) == W
    hm.close()
    topo = LN.wide_out_topology(W + 1)
    err = _refused(LN.write_header_only(os.path.join(tmp_models, "limit_out_524289.bin"), topo, full_layers=3))
    assert err.code == api.FDNN_E_FORMAT and "524289" in str(err) and "524288 outputs" in str(err), str(err)
    # (a hidden width of 32 784 is refused only after the layers have been read -- 4 GB of weights: not built here)
