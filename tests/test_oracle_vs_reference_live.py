"""The CPU oracle against the compiled reference in one process, bit for bit.  Runs only where oracle/_ref/ has been built (the
oracle/Makefile recipe, which needs the reference's sources); skipped, with that reason, everywhere else.  No GPU.

Two parts:

  families   every family of tests/ref_families.py at every frame-block size: multipliers, int8 weights, l0_lin, every u8
             layer, np.float32(acc) against the float accumulator taps, logits AND the soft-max rows (dense and lazy) equal
             as bits -- both sides use one libm here, the assertion tests/golden/make_golden.py makes for the full net;
  sweep      SWEEP_NETS seeded random nets within the loader's rules: hidden width a multiple of 16 up to 512, 2 to 6 int8
             hidden layers, output width 1 .. 1100, input width 4 .. 600, int8 weights of std 0.05 / 0.3 / 0.5, cut-off
             1 / 2 / 3 / 4, 1 .. 24 rows, frame-block size 1 .. 16, both layer-0 flavours, dense and lazy (random masks with
             an all-off, a one-node and an all-on row).  A failure names the seed and the first differing (stage, layer,
             frame, node).

SWEEP_NETS = 1200 was chosen so that this file takes about a minute: measured 48 s to 65 s for the whole file over three runs
(the families about 15 s, the sweep the rest) on the machine the fixtures were generated on."""
import os

import numpy as np
import pytest

import ref_families as RF
from fast_dnn_amd import formats as F
from oracle import oracle as O

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(O.REF_DIR, "libfastdnn_ref.so")),
                                reason="oracle/_ref/libfastdnn_ref.so is absent: the reference was not built on this machine")

SWEEP_NETS = 1200
SWEEP_PARTS = 12


@pytest.fixture(scope="module")
def refs():
    return {False: O.RefLib(), True: O.RefLib(fma=True)}


@pytest.mark.parametrize("name,block", RF.CASES, ids=RF.CASE_IDS)
def test_family_live(tmp_models, refs, name, block):
    fam = RF.FAMILIES[name]
    path = RF.model(fam, tmp_models)
    probe = O.Oracle(path, fam.cutoff)
    in_dim, out_dim = probe.in_dim, probe.out_dim
    probe.close()
    x = RF.features(fam, in_dim)
    m = RF.masks(fam, out_dim) if fam.lazy else None
    rt = RF.reference_taps(refs[fam.fma], fam, path, x, block, m)
    for sse in (True, False):  # the oracle's pmaddubsw path and its scalar statement of the pair saturation
        d = RF.live_difference(rt, RF.oracle_taps(O.Oracle, fam, path, x, block, m, sse=sse))
        assert d is None, f"oracle ({'sse' if sse else 'scalar'}) != reference on [{name}] at block size {block}: {d}"


def sweep_case(seed):
    """-> (Family, FloatNet, block, masks or None) of one sweep seed."""
    rng = np.random.default_rng(seed)
    H = 16 * int(rng.integers(1, 33))
    topo = [int(rng.integers(4, 601))] + [H] * (int(rng.integers(2, 7)) + 1) + [int(rng.integers(1, 1101))]
    w_std = float(rng.choice([0.05, 0.3, 0.5]))
    fam = RF.Family(f"sweep seed {seed}", ("synth", topo, dict(seed=seed, w_std=w_std)), seed, int(rng.integers(1, 25)),
                    cutoff=float(rng.choice([1.0, 2.0, 3.0, 4.0])), fma=bool(rng.integers(0, 2)))
    block = int(rng.integers(1, 17))
    m = None
    if rng.integers(0, 2):
        m = (rng.random((fam.rows, topo[-1])) < 0.4).astype(np.int8)
        for r, row in enumerate((0, 1, 2)[:fam.rows]):
            m[row] = (0, 0, 1)[r]
        if fam.rows > 1:
            m[1, -1] = 1
    return fam, F.synth_net(topo, seed=seed, w_std=w_std), block, m


@pytest.mark.parametrize("part", range(SWEEP_PARTS))
def test_sweep(tmp_path, refs, part):
    path = str(tmp_path / "sweep.bin")
    for seed in range(part, SWEEP_NETS, SWEEP_PARTS):
        fam, net, block, m = sweep_case(10_000 + seed)
        F.write_model_bin(path, net)
        in_dim = -(-net.layers[0].weights.shape[1] // 4) * 4   # the loader pads the input width to whole SSE vectors
        x = F.synth_features(fam.rows, in_dim, seed=fam.seed, pad_from=None)
        rt = RF.reference_taps(refs[fam.fma], fam, path, x, block, m)
        ot = RF.oracle_taps(O.Oracle, fam, path, x, block, m)
        d = RF.live_difference(rt, ot)
        assert d is None, (f"oracle != reference, sweep seed {10_000 + seed} (topology {fam.net[1]}, w_std {fam.net[2]['w_std']}, cut-off {fam.cutoff}, "
                           f"fma {fam.fma}, rows {fam.rows}, block {block}, {'lazy' if m is not None else 'dense'}): {d}")
