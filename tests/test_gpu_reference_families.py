"""The library against what the compiled reference RECORDED (tests/golden/families/*.npz, tests/ref_families.py), with no oracle
in between, on every family but `extreme_acc` and `wide19` (tests/test_gpu_model_limits.py holds those to the oracle on the
same nets, tests/test_oracle_families.py the oracle to the reference).

Per family, at <= 64 frames, loaded with the family's cut-off and layer-0 flavour:
  forwardTaps    l0_lin equal as bits (any NaN equals any NaN: the device's NaN need not carry an x86 NaN's sign), every u8
                 layer equal, np.float32(acc_hid / acc_out) equal to the reference's float accumulator taps as bits;
  calculate      the production instances: <= 2e-6 from the recorded rows (the project's bar), NaN positions equal, the exact
                 zeros of tail/ovf and tail/tot equal, and on lad/* and tail/und softmax_ref.check against float64 of the
                 recorded logits with the c_e of the exp path the launch recorder shows;
  lazy families  calculateLazy(masks=..) and row 5 through a LazyContext frame by frame: <= 2e-6 from the recorded lazy rows,
                 row 0 a constant, masked-out entries of a row all equal.

Which kernel instance runs is the dispatch ledger's business, not this file's: these sizes take the small-batch kernels and
the 32-frame tiles.  `switch.k2048` (16 frames of [432, 2048 x 3, 8000]) is in: its case takes about two seconds.

A failure here that the oracle-based tests do not show means the oracle and the reference disagree on that family;
tests/test_oracle_families.py must then be red as well.  If it is green, this test is wrong."""
import numpy as np
import pytest

import ref_families as RF
import softmax_ref as SR
from conftest import golden
from dispatch_ledger import TIGHT, _masked_out_ok, launched
from fast_dnn_amd import api, formats as F

pytestmark = pytest.mark.gpu

GPU_NAMES = [n for n in RF.NAMES if RF.FAMILIES[n].gpu]
TAP_STAGES = ("l0_lin", "u8_acts", "acc_hid", "acc_out")
INFINITE_TOTAL = ("tail/ovf", "tail/tot")   # the reference's zeros come from 1 / inf, not from an exp that underflows


def exp_path(ran):
    """The exp path (softmax_ref.C_E_PATH) of the output instances among the launched names."""
    if any(n.startswith("ppo.") for n in ran):
        return "v_exp.ppo"
    if any(n.startswith("small.out") for n in ran):
        return "exp2.small"
    assert any(n.startswith("gemm.out") for n in ran), f"no output instance among {sorted(ran)}"
    return "exp2.packed"


@pytest.mark.parametrize("name", GPU_NAMES)
def test_library_equals_the_recorded_reference(tmp_models, name):
    fam = RF.FAMILIES[name]
    g = golden(fam.fixture)
    path = RF.model(fam, tmp_models)
    assert F.sha256_file(path) == str(g["model_sha256"])
    dnn = api.QuantizedDnn.loadFromFile(path, fam.cutoff)
    try:
        dnn.setInputLayerFma(fam.fma)
        x = RF.features(fam, dnn.inputDimension())
        assert RF.sha(x) == str(g["x_sha256"])
        t = dnn.forwardTaps(x)
        RF.compare(fam, g, t, "forwardTaps", canonical_nan=True, stages=TAP_STAGES)
        if fam.inputs == "hostile":
            print(f"\n[families] {name}: l0_lin NaN bits: {RF.first_difference('l0_lin', t['l0_lin'], g['l0_lin']) or 'the recorded ones'}", flush=True)
        for block in fam.blocks:
            p, ran = launched(dnn.calculate, x, block)
            err = RF.compare_rows(fam, g, p, f"calculate b{block}", TIGHT, zeros=name in INFINITE_TOTAL, row_sums=False)
            print(f"\n[families] {name} b{block}: |p - recorded| {err:.3e}; {exp_path(ran)}", flush=True)
            if fam.rel:
                RF.relative_ok(fam, g, p, f"calculate b{block}", SR.C_E_PATH[exp_path(ran)])
        if fam.lazy:
            m = g["masks"]
            lazy, ran = launched(dnn.calculateLazy, x, masks=m)
            RF.compare_rows(fam, g, lazy, "calculateLazy", TIGHT, key="lazy", zeros=False)
            assert (lazy[0] == lazy[0, 0]).all(), f"[{name}]: the all-off row is not a constant"
            _masked_out_ok(lazy, m, f"[{name}] calculateLazy")
            ctx = dnn.getNewLazyContext(fam.rows)
            try:
                ctx.calculateUntilOutput(x)
                rows = np.stack([ctx.calculateForOutputNodes(m[f]) for f in range(6)])
            finally:
                ctx.delete()
            g6 = {"lazy": g["lazy"][:6]}
            RF.compare_rows(fam, g6, rows, "LazyContext rows 0 .. 5", TIGHT, key="lazy", zeros=False)
            assert (rows[0] == rows[0, 0]).all()
            _masked_out_ok(rows, m[:6], f"[{name}] LazyContext")
    finally:
        dnn.delete()
