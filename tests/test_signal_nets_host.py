"""The conditions of tests/signal_nets.py, asserted case by case on the CPU oracle alone (no GPU): without them
tests/test_gpu_signal_nets.py could pass on nets whose frames all look alike.  Prints the figures (-s) that DESIGN.md quotes."""
import numpy as np
import pytest

import signal_nets as SN
from oracle.oracle import Oracle

CASES = SN.cases()


def test_the_grid_keeps_every_class_the_tile_and_the_output_forms_need():
    K = {SN.GRID[n][0][1] for n in SN.GRID}
    assert {16, 48, 240, 256, 272, 512, 1024, 2032, 2048} <= K      # a slice a chunk short, a chunk over, half the waves dead
    assert {1, 3, 4, 31} <= {SN.GRID[n][0][-1] for n in SN.GRID}    # output widths the post-soft-max forms never followed
    frames = {SN.GRID[n][1] for n in SN.GRID}
    assert {31, 33, 63, 65, 97, 129, 161} <= frames and {321, 641, 700} <= frames
    assert len(SN.GRID) <= 20
    for name, raw in SN.RAW_DIM.items():
        assert SN.GRID[name][0][0] in (11 * raw, 432)
    # every case has both modes, but for the widths whose walk-free variant is stated as left out
    assert set(CASES) == {(n, m) for n in SN.GRID for m in SN.MODES} - {(n, "nosat") for n in SN.NOSAT_LEFT_OUT}
    assert set(SN.NOSAT_LEFT_OUT) <= {n for n in SN.GRID if SN.GRID[n][0][1] in (16, 48, 64)}


@pytest.mark.parametrize("name,mode", CASES, ids=[SN.case_id(*c) for c in CASES])
def test_the_case_meets_its_conditions(tmp_models, name, mode):
    topo, n, kw = SN.recipe(name, mode)
    orc = Oracle(SN.path(name, mode, tmp_models))
    x = SN.features(name)
    assert x.shape == (n, topo[0]) and (x != 0).all()
    f = SN.figures(orc, x)
    O = topo[-1]
    risky = [orc.risky_pairs(j) for j in range(1, orc.n_layers)]
    _, (frames, med, values) = f["signal"]
    print(f"\n[signal] {SN.case_id(name, mode)} {topo} n {n} scales {kw['w0_std']}/{kw['w_std']}: distinct rows {frames}, median range {med}, "
          f"values {values}, roll share {f['roll']:.2f}, events {f['events']}, risky pairs {risky}, top-k rows kept {f['topk']}, "
          f"arg-max runs {SN.arg_max_runs(f['probs'])}", flush=True)
    # signal
    SN.assert_keeps_signal(f["taps"]["u8_acts"][-1], SN.case_id(name, mode))
    if O > 1:
        assert f["roll"] > SN.MIN_ROLL_SHARE, f"rolling the hidden rows by one frame moves only {f['roll']:.1%} of the probabilities"
    else:
        assert (f["probs"] == 1.0).all()  # exempt: the only probability is 1
    # saturating pairs
    if mode == "gauss":
        assert f["events"] > 0 and risky[-1] > 0, (f["events"], risky)
    else:
        assert f["events"] == 0 and risky[-1] == 0, (f["events"], risky)
    # finite output
    assert f["nan"] == 0 and np.isfinite(f["probs"]).all()
    # top-k
    assert set(f["topk"]) == set(SN.topk_ks(O))
    for k, share in f["topk"].items():
        assert share >= SN.MIN_TOPK_ROWS, f"top-{k}: only {share:.1%} of the rows have a gap above {SN.TOPK_GAP}"
    orc.close()


def test_the_default_scale_does_not_keep_its_signal(mid_model_path):
    """Information for the reader: the suite's `mid` net (432 -> 3 x 256 -> 1000 at w0_std 0.02, w_std 0.05) fails the signal
    condition by a wide margin, so the grid's scales are not a matter of taste."""
    orc = Oracle(mid_model_path)
    x = SN.features("k256", 200)  # 432 inputs
    _, t = orc.calculate(x, taps=True)
    ok, (frames, med, values) = SN.signal_ok(t["u8_acts"][-1])
    best = orc.calculate(x).argmax(axis=1)
    print(f"\n[signal] mid at the default scale: distinct rows {frames}, median range {med}, values {values}, arg-max nodes {np.unique(best).size}")
    assert not ok and med <= 8, (frames, med, values)
    orc.close()
