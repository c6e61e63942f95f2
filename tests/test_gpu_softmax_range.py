"""The soft-max over exp's range, one case per separately written exp / scale path, against exp(z - max) / sum in float64
within the relative bound of tests/softmax_ref.py -- and the ends of that range against the oracle, exactly.

The ledger's nets give logits of a few units; here the output biases are a shuffled ladder over [-40, 20] ('lad/W', 'ladfull':
tests/dispatch_ledger.py), so exp's argument covers 87 units, four fifths of a row lie below the suite's 2e-6 absolute bar and
every probability is still a normal fp32: no entry may take check()'s second class (share == 0).  Every case runs under the
launch recorder and asserts the exact set of instances it launched -- the sizes are the smallest the selection rules allow for
each instance.  Integer state and tap logits are compared with the oracle bit for bit on the way.

Tails ('tail/ovf|tot|und', 'tailfull/ovf': output weights / 256, logits = biases to 0.05):
  ovf  four logits at 95: exp = +inf, total = +inf, 1 / total = 0: those four NaN, every other entry 0 -- the oracle's row;
  tot  64 logits at 87: every exp finite, the total +inf: every entry 0 -- the oracle's row;
  und  a ladder over [-120, 0]: probabilities below 2^-126 beside normal ones; the share of the second class equals the share
       computed from the float64 reference alone.
Rows whose every logit is below -87 are not tested: the hardware exp flushes the whole row, the total is 0 and the row NaN,
where glibc's expf still returns denormals (a documented deviation, not pinned as expected behaviour)."""
import numpy as np
import pytest

import dispatch_ledger as L
import softmax_ref as SR
from fast_dnn_amd import api

pytestmark = pytest.mark.gpu

E = L.EXPECT
_ANYW_545 = {"gemm.out.ft32.anyw", "gemm.out.ft32.masked_anyw", "l0.tile32.prod", "maskpack.rows", "norm.rows", "small.hid.nt32.prod"}

# id: (net, n, entry, exp path (softmax_ref.C_E_PATH), the instances the case is for, the exact launched set, modes)
RANGE = {
    "small.n33":          ("lad/256", 33, "prod", "exp2.small", ("small.out.prod", "small.out.masked", "norm.small"), E["n256.small.n33"], dict(fuse=0)),
    "small.n32":          ("lad/251", 32, "prod", "exp2.small", ("small.out.prod", "small.out.masked", "norm.rows"), E["n256.small.n32"], dict(fuse=0)),
    "ft32.plain.n544":    ("lad/256", 544, "prod", "exp2.packed", ("gemm.out.ft32.plain",), E["n256.small_ft32.n544"], dict(fuse=0)),
    "ft32.anyw.n545":     ("lad/251", 545, "prod", "exp2.packed", ("gemm.out.ft32.anyw",), _ANYW_545, dict(fuse=0)),
    "ft32.masked_anyw.n575": ("lad/251", 575, "prod", "exp2.packed", ("gemm.out.ft32.masked_anyw",), E["n256.small_ft32.n575"], dict(fuse=0)),
    "ft32.tap.n1000":     ("lad/256", 1000, "taps", "expf", ("gemm.out.ft32.tap",), E["n256.taps.n1000"], {}),
    "fused.n16512":       ("lad/256", 16512, "prod", "exp2.packed", ("gemm.out.ft128.bk128.fused", "gemm.out.ft128.bk128.fused_masked"),
                           E["n256.ft128.fused.n16512"], {}),
    "fused_anyw.n16513":  ("lad/251", 16513, "prod", "exp2.packed", ("gemm.out.ft128.bk128.fused_anyw", "gemm.out.ft128.bk128.fused_masked_anyw"),
                           E["n256.ft128.fused.n16639"], {}),
    "server.n300":        ("lad/256", 300, "server", "exp2.small", ("small.out.prod", "norm.small"), E["entry.server.n300"], dict(fuse=0)),
    "lazy_bits.n300":     ("lad/256", 300, "lazy_bits", "exp2.small", ("compact", "small.out.masked"), E["entry.lazy_bits.n300"], {}),
    "full.ppo.n513":      ("ladfull", 513, "dense_device", "v_exp.ppo", ("ppo.out.fix",), E["full.ppo.fix.n513"], dict(ppo=1)),
    "full.ppo.n641":      ("ladfull", 641, "dense_device", "v_exp.ppo", ("ppo.out.fix",), E["full.ppo.fix.n641"], dict(ppo=1)),
    "full.fused320.n10000": ("ladfull", 10000, "prod", "exp2.packed", ("gemm.out.ft320.fused", "gemm.out.ft320.fused_masked"),
                             E["full.fused320.n10000"], dict(chain=(0, 0))),
}
_TAIL_PATHS = {
    "small.n33":      (33, "exp2.small", ("small.out.prod",), E["n256.small.n33"], dict(fuse=0)),
    "ft32.n544":      (544, "exp2.packed", ("gemm.out.ft32.plain",), E["n256.small_ft32.n544"], dict(fuse=0)),
    "fused.n16512":   (16512, "exp2.packed", ("gemm.out.ft128.bk128.fused",), E["n256.ft128.fused.n16512"], {}),
    "unfused.n16512": (16512, "exp2.packed", ("gemm.out.ft128.bk128.plain", "norm.rows"), E["n256.ft128.unfused.n16512"], dict(fuse=0)),
}
TAILS = {f"{net}.{pid}": (f"tail/{net}", n, "prod", path, must, want, modes)
         for net in ("ovf", "tot", "und") for pid, (n, path, must, want, modes) in _TAIL_PATHS.items()}
TAILS["ovf.full.ppo.n513"] = ("tailfull/ovf", 513, "dense_device", "v_exp.ppo", ("ppo.out.fix",), E["full.ppo.fix.n513"], dict(ppo=1))


@pytest.fixture(scope="module", autouse=True)
def models():
    yield
    api.launch_record(False)
    L.release_models()


def run(cid, spec):
    """The case through the ledger's runner (dispatch_ledger.run_case: the recorder on, the case's modes set and reset, the
    ledger's features and masks for that size, integer state against the oracle bit for bit) as an integer-only case -- the
    soft-max checks are this file's -- with the exact launched set asserted -> (what the entry returned, the rows compared, the
    oracle's accumulators, probabilities and masked probabilities on those rows, the masks, the oracle)."""
    net, n, entry, path, must, want_names, modes = spec
    case = L.Case(cid, net, n, entry, must, integer_only=True, tile=320, **modes)
    if net.startswith(("lad/", "tail/")) and entry == "prod":
        case.chain = (0, 0)  # as the ledger's n256 cases: one launch per hidden layer
    assert set(must) <= want_names
    d = {}
    try:
        names = L.run_case(case, detail=d)
    finally:
        api.launch_record(False)
    assert names == want_names, f"{cid}: launched but not expected: {sorted(names - want_names)}; expected but not launched: {sorted(want_names - names)}"
    got, idx, masks, orc = d["got"], d["idx"], d["masks"], d["orc"]
    if entry == "taps":
        wt = d["wt"]
        assert np.array_equal(got["logits"].view(np.uint32), wt["logits"].view(np.uint32)), f"{cid}: logits differ from the oracle"
        SR.logits(wt["acc_out"], SR.coef_of(orc), orc.layer_bias(orc.n_layers - 1), tap=wt["logits"])
        return {"dense": got["probs"]}, idx, wt["acc_out"], d["want"], None, None, orc
    want_lazy = orc.output_mt(d["hid"], masks=masks[idx]) if "lazy" in got else None
    return got, idx, d["acc"], d["want"], want_lazy, masks, orc


def outputs(got, idx, acc, want, want_lazy, masks, orc):
    """(name, the library's rows, the reference's fp32 logits, the oracle's rows, the rows' masks) per output the case returned."""
    coef, bias = SR.coef_of(orc), orc.layer_bias(orc.n_layers - 1)
    if "dense" in got:
        yield "dense", got["dense"][idx], SR.logits(acc, coef, bias), want, None
    if "lazy" in got:
        yield "lazy", got["lazy"][idx], SR.logits(acc, coef, bias, masks=masks[idx]), want_lazy, masks[idx]


@pytest.mark.parametrize("cid", list(RANGE))
def test_range_case_is_within_the_relative_bound(cid):
    """Prints softmax_ref.measure()'s figures (run with -s): what profiles/LABBOOK.md, 'Soft-max: c_e per exp path', records."""
    spec = RANGE[cid]
    verify_range(cid, spec, run(cid, spec))


def verify_range(cid, spec, res):
    rows_pad = SR.rows_pad_of(res[-1].out_dim)
    for name, p, z, want, m in outputs(*res):
        if m is not None:
            L._masked_out_ok(p, m, cid)
        print(f"\n[softmax-range] {cid} {name} path {spec[3]} rows {p.shape[0]}: {SR.measure(p, z, rows_pad)}", flush=True)
        assert not np.isnan(want).any() and (SR.softmax64(z) >= SR.TINY).all()  # the fixture's premise (tests/test_softmax_ref_host.py)
        share = SR.check(p, z, rows_pad, f"{cid} {name}", c_e=SR.C_E_PATH[spec[3]])
        assert share == 0.0, f"{cid} {name}: {share:.3%} of the entries took the second class"


@pytest.mark.parametrize("cid", list(TAILS))
def test_tail_case(cid):
    spec = TAILS[cid]
    verify_tail(cid, spec, run(cid, spec))


def verify_tail(cid, spec, res):
    rows_pad = SR.rows_pad_of(res[-1].out_dim)
    kind = spec[0].split("/")[1]
    for name, p, z, want, m in outputs(*res):
        # rows the oracle ends in NaN or all-zero (an infinite exp or total): exactly the oracle's row
        special = np.isnan(want).any(1) | (want == 0).all(1)
        if kind in ("ovf", "tot") and name == "dense":
            assert special.all(), f"{cid}: the net does not overflow every dense row"
        if kind == "ovf" and name == "dense":
            assert (np.isnan(want).sum(1) == 4).all() and (want[~np.isnan(want)] == 0).all()
        assert np.array_equal(p[special], want[special], equal_nan=True), f"{cid} {name}: overflowing rows differ from the oracle"
        rest = ~special  # (a lazy row whose large logits are all masked out is an ordinary row)
        if kind == "und":
            assert rest.all()
        if rest.any():
            if m is not None:
                L._masked_out_ok(p[rest], m[rest], cid)
            p64 = SR.softmax64(z[rest])
            share = SR.check(p[rest], z[rest], rows_pad, f"{cid} {name}", c_e=SR.C_E_PATH[spec[3]])
            assert share == (p64 < SR.TINY).mean()
            if kind == "und":
                assert 0.05 < share < 0.35  # (dense 28 %; lazy rows: the masked-out 60 % are 1 / total each)
                assert (z[rest].max(1) > -1.0).all()  # no row near the all-underflow deviation
                print(f"\n[softmax-range] {cid} {name}: second class {share:.3%}; zeros {float((p[rest] == 0).mean()):.3%}; "
                      f"denormals {float(((p[rest] > 0) & (p[rest] < SR.TINY)).mean()):.3%}", flush=True)
