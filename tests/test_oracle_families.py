"""The CPU oracle (oracle/fdnn_oracle.c) against what the compiled reference recorded for every family of
tests/ref_families.py (tests/golden/make_family_golden.py -> tests/golden/families/*.npz).  No GPU, no reference needed.

Every GPU test holds a kernel to the oracle; this file is what holds the oracle to the reference on the nets and inputs those
tests use -- and would turn red if a later edit to the oracle drifted.  Per family and frame-block size, equal as bits: the
regenerated model's sha256, multipliers and int8 weights, l0_lin, every u8 layer, np.float32(acc) against the reference's float
accumulator taps, the logits; integer equality of the accumulators wherever the tap's magnitude is below 2^24; NaN and zero
positions of the soft-max rows; the rows within 1e-6 (tests/test_oracle_golden.py's bar: another image's libm may differ in the
last place).  That absolute bar is blind to most of a `lad` row and to all of `tail/und`, so there the recorded rows AND the
oracle's rows must each pass softmax_ref.check against the float64 soft-max of the recorded logits (c_e of the expf path).

test_fixture_is_not_blind repeats, from the fixture alone, the conditions the generator asserted on the reference's data."""
import os

import numpy as np
import pytest

import ref_families as RF
import softmax_ref as SR
from conftest import GOLDEN, golden
from fast_dnn_amd import formats as F
from oracle.oracle import Oracle

C_E = SR.C_E_PATH["expf"]


def test_every_family_has_a_fixture_within_the_size_rule():
    for fam in RF.FAMILIES.values():
        p = os.path.join(GOLDEN, fam.fixture)
        assert os.path.exists(p), f"{fam.name}: {fam.fixture} is missing (tests/golden/make_family_golden.py)"
        assert os.path.getsize(p) <= RF.MAX_FIXTURE_BYTES, (fam.name, os.path.getsize(p))
        g = golden(fam.fixture)
        assert int(g["rows"]) == fam.rows <= 64 and tuple(g["blocks"]) == fam.blocks
        assert float(g["cutoff"]) == fam.cutoff and bool(g["fma"]) == fam.fma
    assert os.path.getsize(os.path.join(GOLDEN, "quantizer_wide.npz")) <= RF.MAX_FIXTURE_BYTES


@pytest.mark.parametrize("name,block", RF.CASES, ids=RF.CASE_IDS)
def test_oracle_equals_the_recorded_reference(tmp_models, name, block):
    fam = RF.FAMILIES[name]
    g = golden(fam.fixture)
    path = RF.model(fam, tmp_models)
    assert F.sha256_file(path) == str(g["model_sha256"]), f"{name}: the regenerated .bin is not the recorded one (a generator drifted, not the oracle)"
    o = Oracle(path, fam.cutoff)
    in_dim, out_dim = o.in_dim, o.out_dim
    o.close()
    x = RF.features(fam, in_dim)
    assert RF.sha(x) == str(g["x_sha256"]), f"{name}: the regenerated input rows are not the recorded ones"
    m = RF.masks(fam, out_dim) if fam.lazy else None
    if m is not None:
        assert np.array_equal(m, g["masks"])
    for sse in (True, False):
        what = f"oracle b{block} {'sse' if sse else 'scalar'}"
        t = RF.oracle_taps(Oracle, fam, path, x, block, m, sse=sse)
        assert np.array_equal(t["mult"].view(np.uint32), g["mult"].view(np.uint32)), f"{what} [{name}]: multipliers {t['mult']} against {g['mult']}"
        assert list(t["wq_sha256"]) == list(g["wq_sha256"]), f"{what} [{name}]: int8 weights differ"
        RF.compare(fam, g, t, what)
        if fam.lazy:
            RF.compare_rows(fam, g, t["lazy"], what, RF.ABS_BAR, key="lazy")
        if fam.rel:
            RF.relative_ok(fam, g, g["probs"], "recorded reference", C_E)
            RF.relative_ok(fam, g, t["probs"], what, C_E)


@pytest.mark.parametrize("name", [n for n in RF.NAMES if RF.FAMILIES[n].props])
def test_fixture_is_not_blind(tmp_models, name):
    """The family's condition holds on the RECORDED data: planted saturation events in every int8 layer, accumulator taps beyond
    2^24, an FMA layer 0 that differs from the plain one in >= 25 % of its entries, the NaN / zero / sub-normal rows of the
    tails, hostile rows whose bytes depend on the hostile element, the constant all-off lazy row, cut-offs that change the weights."""
    fam = RF.FAMILIES[name]
    g = golden(fam.fixture)
    wq = None
    if "events" in fam.props and not fam.sample:
        wq = RF.int8_weights(RF.model(fam, tmp_models), fam, Oracle.quantize)
        assert [RF.sha(w) for w in wq] == list(g["wq_sha256"])  # the weights the events are counted with are the recorded ones
    RF.properties(fam, g, wq=wq, plain_l0=g["plain_l0_lin"] if fam.fma else None, base=golden(RF.FAMILIES["plain"].fixture))


def test_quantizer_wide_cases():
    g = golden("quantizer_wide.npz")
    assert len(g["names"]) == 16
    with np.errstate(all="ignore"):
        for name in g["names"]:
            wq, mult = Oracle.quantize(g[f"{name}_w"], float(g[f"{name}_cut"]))
            assert (wq == g[f"{name}_wq"]).all(), name
            assert np.array_equal(np.float32(mult), g[f"{name}_mult"], equal_nan=True), (name, mult, float(g[f"{name}_mult"]))
