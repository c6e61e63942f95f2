"""The families of nets and inputs on which the oracle (oracle/fdnn_oracle.c) is pinned to the reference itself.  Plain helper
module: numpy only, no GPU, no fixture.

Every GPU test holds a kernel to the oracle; this table names the nets and inputs those tests trust, built ONLY from the
helpers they use (formats.synth_net / synth_features / generate_masks, sat_switch, limit_nets, signal_nets,
dispatch_ledger.net_path), so that what is recorded from the reference (tests/golden/make_family_golden.py ->
tests/golden/families/*.npz) is what the suite relies on.  Users:

  tests/golden/make_family_golden.py     drives the compiled reference, asserts each family's property on its data, stores it
  tests/test_oracle_families.py          the oracle against the stored data (everywhere)
  tests/test_oracle_vs_reference_live.py the oracle against the reference in one process (where oracle/_ref/ was built)
  tests/test_gpu_reference_families.py   the library against the stored data, no oracle in between

A recipe (Family) states the net, the feature seed, the rows (<= 64), the frame-block sizes, the weight cut-off, the layer-0
flavour and whether masks go with it.  record() turns the reference's taps into a fixture; compare() holds any other taps
(the oracle's, the library's) to a fixture and names the first differing (stage, layer, frame, node); properties() are the
conditions without which a family's fixture would be blind -- asserted on the reference's data alone.

The float-tap rule: the reference's accumulator tap is float(int32) (quantizedNodeSum returns a float), so accumulators are
compared as np.float32(acc) against the tap bit for bit, and as integers only where the tap's magnitude is below 2^24."""
import hashlib
from dataclasses import dataclass

import numpy as np

import softmax_ref as SR

MAX_FIXTURE_BYTES = 464 * 1024   # no new fixture is larger than the largest one committed before (tiny.npz)
ABS_BAR = 1e-6                   # tests/test_oracle_golden.py's bar for soft-max rows across images (another libm's last place)
EXACT = 1 << 24                  # below this magnitude a float tap holds its int32 exactly


def _F():
    from fast_dnn_amd import formats as F

    return F


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------------------ hostile rows
def hostile_block(x, rng, unit=32):
    """Rows a 24-bit integer image of a frame cannot represent, written into x in place, `unit` rows per kind (the layout of
    tests/test_gpu_production_shapes.py::test_int8_screening_with_hostile_rows at unit = 32): one element 10^6 times the
    rest (2 units), all-zero rows, denormal rows, tiny and huge uniform scales, one row each with +inf, -inf, NaN and
    3e38 everywhere, rows whose halves cancel (2 units), rows of exact ties.  Needs 9 * unit + 8 rows.
    -> {name: row} of the four rows that carry inf / NaN / 3e38, and the column of the planted element (None: the whole row)."""
    u, d = int(unit), x.shape[1]
    assert x.shape[0] >= 9 * u + 8 and d >= 12
    x[0:2 * u, 7] = 1.0e6                                   # one dominant element
    x[2 * u:3 * u] = 0.0                                    # empty rows
    x[3 * u:4 * u] = (rng.standard_normal((u, d)) * 1e-41).astype(np.float32)   # denormal inputs
    x[4 * u:5 * u] *= np.float32(1e-12)
    x[5 * u:6 * u] *= np.float32(1e12)
    x[6 * u, 3] = np.inf
    x[6 * u + 1, 5] = -np.inf
    x[6 * u + 2, 11] = np.nan
    x[6 * u + 3] = np.float32(3.0e38)
    lo, hi, half = 6 * u + 8, 8 * u + 8, d // 2
    x[lo:hi, :half] = -x[lo:hi, half:2 * half]              # (shift/scale sit between this and the layer, so only near-cancelling)
    x[hi:hi + u] = np.round(x[hi:hi + u] * 4) / 4           # many exact ties in the products
    return {"inf": (6 * u, 3), "ninf": (6 * u + 1, 5), "nan": (6 * u + 2, 11), "huge": (6 * u + 3, None)}


HOSTILE_UNIT = 4     # the family's layout: 44 rows of kinds, 60 rows in all, then the four cleaned copies


def hostile_features():
    """64 rows: synth_features(60) under hostile_block(unit = 4), then rows 60 .. 63 = the inf, -inf, NaN and 3e38 rows with
    the planted element (the whole row for 3e38) set to 0 -> (x, planted {name: (row, column)}, cleaned {name: row})."""
    x = np.concatenate([_F().synth_features(60, 432, seed=31), np.zeros((4, 432), np.float32)])
    planted = hostile_block(x[:60], np.random.default_rng(5), unit=HOSTILE_UNIT)
    cleaned = {}
    for i, (name, (row, col)) in enumerate(planted.items()):
        x[60 + i] = x[row]
        if col is None:
            x[60 + i] = 0.0
        else:
            x[60 + i, col] = 0.0
        cleaned[name] = 60 + i
    return x, planted, cleaned


# ----------------------------------------------------------------------------------------------------------------- recipes
@dataclass(frozen=True)
class Family:
    name: str
    net: tuple                 # ("synth", topology, synth_net keywords) | ("switch", kind) | ("deep", n_hidden) | ("wide_out", W) |
    #                            ("extreme_acc",) | ("ledger", kind)
    seed: int                  # of the features (and of the masks and the column sample)
    rows: int
    blocks: tuple = (10,)      # frame-block sizes: blocking never changes a result, every block size is held to the one fixture
    cutoff: float = 3.0
    fma: bool = False          # layer 0 as the reference computes it when its mul + add fuse
    inputs: str = "synth"      # synth | x50 | hostile | switch (sat_switch.features under crowded_switches) | signal (signal_nets.features)
    lazy: bool = False         # masks: row 0 all off, row 1 only the last node on, row 2 all on, the rest generate_masks(.., 0.4, 0.05)
    sample: int = 0            # > 0: too large to store -- integer state as sha256, float state at `sample` seeded columns
    props: tuple = ()          # the conditions of properties()
    rel: bool = False          # rows also held to softmax_ref's relative bound against float64 of the recorded logits
    gpu: bool = True           # in tests/test_gpu_reference_families.py

    @property
    def fixture(self):
        return "families/" + self.name.replace("/", "_").replace("signal.", "signal_", 1) + ".npz"


FAMILIES = {}


def _fam(name, net, seed, rows, **kw):
    assert name not in FAMILIES and rows <= 64
    FAMILIES[name] = Family(name, net, seed, rows, **kw)


IN_TOPO = lambda d: [d, 144, 144, 144, 40]      # tests/test_gpu_parity.py::test_input_widths_and_the_chain_image_padding
# the plain net: Gaussian, its int8 layers with std 1.25, so that their weights reach beyond every cut-off the tools use
# (the quantizer clamps at +-cutoff in absolute terms: a net of std 0.05 quantizes alike under cut-offs 2, 3 and 4)
PLAIN = ("synth", [432, 128, 128, 128, 252], dict(seed=91, w_std=1.25))

_fam("plain", PLAIN, 101, 40)
_fam("hostile", PLAIN, 31, 64, blocks=(10, 1), inputs="hostile", props=("hostile",))
for _h in (16, 144, 272):                         # tests/test_gpu_parity.py: the hidden widths either side of a 128-node tile
    _fam(f"hid{_h}", ("synth", [432, _h, _h, _h, 52], dict(seed=20 + _h)), 9, 33)
for _d in (20, 64, 100, 440, 448):
    _fam(f"in{_d}", ("synth", IN_TOPO(_d), dict(seed=60 + _d)), _d, 33)
for _o, _n in ((37, 33), (101, 33), (1003, 16)):
    _fam(f"out{_o}", ("synth", [432, 128, 128, 128, _o], dict(seed=700 + _o)), _o, _n)
    _fam(f"out{_o}.lazy", ("synth", [432, 128, 128, 128, _o], dict(seed=700 + _o)), _o + 1, _n, lazy=True, props=("lazy",))
# the topology of sat.npz with int8 weights of std 0.3: at 0.05 features x 50 saturate pairs of the first int8 layer only
_fam("x50", ("synth", [432, 128, 128, 128, 200], dict(seed=8, w_std=0.3)), 50, 32, inputs="x50", props=("events",))
for _k, _n in (("k256.w256", 48), ("k256.w252", 48), ("k256.w251", 48), ("tdiv.w252", 64)):
    _fam(f"switch.{_k}", ("switch", _k), 13, _n, inputs="switch", props=("events",))
_fam("switch.k2048", ("switch", "k2048"), 13, 16, inputs="switch", sample=512, props=("events",))
_fam("deep29", ("deep", 29), 3033, 12)
_fam("extreme_acc", ("extreme_acc",), 81, 16, sample=256, props=("extreme",), gpu=False)
_fam("wide19", ("wide_out", 1 << 19), 4, 3, sample=4096, props=("normal",), gpu=False)
_fam("tdiv/200", ("ledger", "tdiv/200"), 200, 32)
_fam("allsat", ("ledger", "allsat"), 17, 32, props=("events",))
_fam("wide/64", ("ledger", "wide/64"), 64, 32)
_fam("d64", ("ledger", "d64"), 41, 32)
_fam("lad/256", ("ledger", "lad/256"), 256, 32, props=("normal",), rel=True)
_fam("lad/251", ("ledger", "lad/251"), 251, 32, props=("normal",), rel=True)
_fam("tail/ovf", ("ledger", "tail/ovf"), 1, 24, props=("ovf",))
_fam("tail/tot", ("ledger", "tail/tot"), 2, 24, props=("tot",))
_fam("tail/und", ("ledger", "tail/und"), 3, 24, props=("und",), rel=True)
_fam("n256/256/nosat", ("ledger", "n256/256/nosat"), 556, 32)
for _d in (20, 64, 100, 440, 448):
    _fam(f"fma.in{_d}", ("synth", IN_TOPO(_d), dict(seed=60 + _d)), _d, 33, blocks=(1, 7, 10), fma=True, props=("fma",))
_fam("fma.in432", PLAIN, 101, 40, blocks=(1, 7, 10), fma=True, props=("fma",))
_fam("fma.in2048", ("ledger", "wide/64"), 64, 32, blocks=(1, 7, 10), fma=True, props=("fma",))
_fam("fma.hostile", PLAIN, 31, 64, blocks=(10, 1), fma=True, inputs="hostile", props=("hostile", "fma"))
_fam("cut2", PLAIN, 101, 40, cutoff=2.0, props=("cutoff",))
_fam("cut4", PLAIN, 101, 40, cutoff=4.0, props=("cutoff",))


def _signal_families():
    """tests/signal_nets.py's grid, both modes: the first min(n, 64) rows of each case's own features.  The wide ones keep hashes
    and 256 sampled columns.  k1024 stays out of the GPU file: the reference's sequential fp32 row total is 2.7e-6 off the
    float64 soft-max on these rows (3.5e-6 over all 641), more than the 2e-6 that file allows between the library and the
    recorded rows; tests/test_gpu_signal_nets.py holds the library to float64 of the oracle's logits on that net instead."""
    import signal_nets as SN

    for name, mode in SN.cases():
        topo, n, kw = SN.recipe(name, mode)
        _fam(f"signal.{name}" + ("" if mode == "gauss" else ".nosat"), ("synth", topo, kw), SN.FEATURE_SEED, min(n, 64), inputs="signal",
             sample=256 if topo[1] >= 512 else 0, props=("signal",), gpu=name != "k1024")


_signal_families()

NAMES = tuple(FAMILIES)
CASES = tuple((n, b) for n in NAMES for b in FAMILIES[n].blocks)    # (family, frame-block size)
CASE_IDS = tuple(f"{n}-b{b}" for n, b in CASES)


# ---------------------------------------------------------------------------------------------------------- nets and inputs
def model(fam, directory):
    """The family's net as a .bin in `directory`, written unless it is there -> path."""
    import limit_nets as LN

    F = _F()
    kind = fam.net[0]
    if kind == "synth":
        topo, kw = fam.net[1], fam.net[2]
        tag = hashlib.sha256(repr((topo, sorted(kw.items()))).encode()).hexdigest()[:12]
        return LN.cached(directory, f"family_{tag}", topo, lambda: F.synth_net(topo, **kw))
    if kind == "switch":
        import sat_switch as SW

        return SW.model_file(directory, fam.net[1])[0]
    if kind == "deep":
        n_hid = fam.net[1]
        return LN.cached(directory, f"limit_deep_{n_hid}x256", LN.deep_topology(n_hid), lambda: LN.deep_net(n_hid))
    if kind == "wide_out":
        W = fam.net[1]
        return LN.cached(directory, f"limit_wide_out_{W}", LN.wide_out_topology(W), lambda: LN.wide_out_net(W))
    if kind == "extreme_acc":
        return LN.extreme_acc_file(directory)[0]
    if kind == "ledger":
        import dispatch_ledger as DL

        return DL.net_path(fam.net[1], directory)
    raise ValueError(fam.net)


def features(fam, in_dim):
    """The family's input rows [rows][in_dim] fp32, from its seed."""
    F = _F()
    if fam.inputs == "hostile":
        x = hostile_features()[0]
    elif fam.inputs == "switch":
        import sat_switch as SW

        x = SW.features(fam.rows, SW.crowded_switches(fam.rows, fam.seed), fam.seed)
    elif fam.inputs == "signal":
        x = F.synth_features(fam.rows, in_dim, seed=fam.seed, pad_from=None)
    else:
        x = F.synth_features(fam.rows, in_dim, seed=fam.seed)
        if fam.inputs == "x50":
            x = (x * 50).astype(np.float32)
    assert x.shape == (fam.rows, in_dim) and x.dtype == np.float32, (fam.name, x.shape)
    return x


def masks(fam, out_dim):
    """Row 0 all off, row 1 only the last node on, row 2 all on, the rest generate_masks(rows - 3, out_dim, 0.4, 0.05)."""
    assert fam.lazy and fam.rows >= 6
    m = np.zeros((fam.rows, out_dim), np.int8)
    m[1, -1] = 1
    m[2] = 1
    m[3:] = _F().generate_masks(fam.rows - 3, out_dim, ratio=0.4, churn=0.05, seed=fam.seed)
    return m


def sample_columns(fam, width):
    """The seeded column sample of a family too large to store: sorted, distinct; the planted rows of extreme_acc among them."""
    rng = np.random.default_rng(fam.seed + width)
    k = min(fam.sample, width)
    cols = rng.choice(width, k, replace=False)
    if fam.net[0] == "extreme_acc":
        import limit_nets as LN

        cols = np.union1d(cols, np.arange(LN.ACC_ROWS))
    return np.sort(cols).astype(np.int64)


# --------------------------------------------------------------------------------------------------------- taps of either side
STAGES = ("l0_lin", "u8_acts", "acc_hid", "acc_out", "logits", "probs")


def reference_taps(ref_lib, fam, path, x, block, m=None):
    """The compiled reference's taps (oracle.RefLib of the family's flavour): float accumulator taps as they are."""
    r = ref_lib.load(path, fam.cutoff)
    try:
        with np.errstate(all="ignore"):
            t = r.forward_taps(x, batch=block)
            if m is not None:
                t["lazy"] = r.lazy(x, m, batch=block)
        t["mult"] = np.array([r.q_mult(j) for j in range(r.n_q)], dtype=np.float32)
        t["wq_sha256"] = np.array([sha(r.q_weights(j)) for j in range(r.n_q)])
        return t
    finally:
        r.close()


def oracle_taps(Oracle, fam, path, x, block, m=None, sse=True):
    """The oracle's taps in the same form; int32 accumulators kept beside their float32 image.  `Oracle`: oracle.Oracle."""
    o = Oracle(path, fam.cutoff)
    Oracle.set_l0_fma(fam.fma)
    try:
        with np.errstate(all="ignore"):
            p, t = o.calculate(x, batch=block, sse=sse, taps=True)
            if m is not None:
                t["lazy"] = o.lazy(x, m, batch=block, sse=sse)
    finally:
        Oracle.set_l0_fma(False)
    t["probs"] = p
    t["mult"] = np.array([o.layer_mult(j) for j in range(1, o.n_layers)], dtype=np.float32)
    t["wq_sha256"] = np.array([sha(o.layer_wq(j)) for j in range(1, o.n_layers)])
    o.close()
    return t


def float_taps(t):
    """acc_hid / acc_out as the reference taps them: np.float32 of the int32 (nothing happens to arrays that are float)."""
    t = dict(t)
    for k in ("acc_hid", "acc_out"):
        if t[k].dtype != np.float32:
            t[k + "_int"] = t[k]
            t[k] = t[k].astype(np.float32)
    return t


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def first_difference(stage, got, want, canonical_nan=False):
    """None where got and want are equal as bits, else 'stage layer L frame F node N: got .. want ..' of the first difference.
    canonical_nan: any NaN equals any NaN (another machine's NaN need not carry this one's sign and payload)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{stage}: shape / type {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    ne = _bits(got) != _bits(want)
    if canonical_nan and got.dtype == np.float32:
        ne &= ~(np.isnan(got) & np.isnan(want))
    if not ne.any():
        return None
    i = tuple(int(v) for v in np.argwhere(ne)[0])
    layer, frame, node = ((0,) * (3 - len(i)) + i)[-3:]
    return f"{stage} layer {layer} frame {frame} node {node}: got {got[i]!r} want {want[i]!r} ({int(ne.sum())} entries differ)"


def live_difference(ref_t, orc_t, stages=STAGES + ("lazy",)):
    """The first stage at which the oracle's taps differ from the reference's as bits (both on one machine: the soft-max
    rows included), or None."""
    o = float_taps(orc_t)
    for k in ("mult", "wq_sha256"):
        if not np.array_equal(ref_t[k], o[k]):
            return f"{k}: {o[k].tolist()} against {ref_t[k].tolist()}"
    for st in stages:
        if st in ref_t:
            d = first_difference(st, o[st], ref_t[st])
            if d:
                return d
    return None


# ------------------------------------------------------------------------------------------------------------------ fixtures
def record(fam, ref_t, model_sha, x, m=None):
    """The reference's taps -> the arrays of the family's fixture (data only)."""
    n = x.shape[0]
    g = dict(model_sha256=model_sha, x_sha256=sha(x), rows=np.int64(n), blocks=np.array(fam.blocks, np.int64),
             cutoff=np.float32(fam.cutoff), fma=np.bool_(fam.fma), mult=ref_t["mult"], wq_sha256=ref_t["wq_sha256"])
    if fam.inputs == "hostile":
        g["x"] = x
    if not fam.sample:
        for st in STAGES:
            g[st] = ref_t[st]
    else:
        for st in STAGES:
            a = ref_t[st]
            if st != "probs":
                g[st + "_sha256"] = np.array([sha(a[j]) for j in range(a.shape[0])]) if a.ndim == 3 else sha(a)
            cols = sample_columns(fam, a.shape[-1])
            g[st + "_cols"] = cols
            g[st + "_sample"] = a[..., cols]
        p = ref_t["probs"]
        g["probs_nan"] = np.argwhere(np.isnan(p)).astype(np.int64)
        g["probs_zero"] = np.argwhere(p == 0).astype(np.int64)
        g["probs_row_sum"] = p.astype(np.float64).sum(axis=1)
        g["probs_min"], g["probs_max"] = np.float32(np.nanmin(p)), np.float32(np.nanmax(p))
        g["acc_big"] = np.int64(sum(int((np.abs(ref_t[k]) >= EXACT).sum()) for k in ("acc_hid", "acc_out")))
        g["acc_max"] = np.float32(max(float(np.abs(ref_t[k]).max()) for k in ("acc_hid", "acc_out")))
        if fam.net[0] == "extreme_acc":
            import limit_nets as LN

            g["acc_planted"] = ref_t["acc_hid"][1][:, :LN.ACC_ROWS]
    if "signal" in fam.props:
        import limit_nets as LN

        g["signal"] = np.array(LN.signal_stats(ref_t["u8_acts"][-1]), np.float64)   # distinct rows, median node range, byte values
    if m is not None:
        g["masks"] = m
        g["lazy"] = ref_t["lazy"]
    return g


def compare(fam, g, t, what, canonical_nan=False, integer_taps=True, probs_bar=ABS_BAR, stages=STAGES):
    """Hold taps `t` (float_taps form) to the fixture `g`: l0_lin, the u8 layers, np.float32(acc) and the logits as bits, integer
    accumulators wherever the tap's magnitude is below 2^24, NaN and zero positions of the rows, the rows within
    `probs_bar`.  -> the largest |p - recorded| seen.  AssertionError names the family, stage, layer, frame and node."""
    t = float_taps(t)
    err = 0.0
    for st in stages:
        if st == "probs":
            continue
        if not fam.sample:
            d = first_difference(st, t[st], g[st], canonical_nan)
        else:
            a = t[st]
            got = np.array([sha(a[j]) for j in range(a.shape[0])]) if a.ndim == 3 else np.array(sha(a))
            d = None if np.array_equal(got, g[st + "_sha256"]) else f"{st}: sha256 differs from the recorded one"
            # (the sample names the place where the hash cannot)
            d = first_difference(st + " (sampled columns)", a[..., g[st + "_cols"]], g[st + "_sample"], canonical_nan) or d
        assert d is None, f"{what} [{fam.name}]: {d}"
        if integer_taps and st in ("acc_hid", "acc_out") and st + "_int" in t:
            want = g[st + "_sample"] if fam.sample else g[st]
            got = t[st + "_int"][..., g[st + "_cols"]] if fam.sample else t[st + "_int"]
            exact = np.abs(want) < EXACT
            d = first_difference(st + " (int32)", np.where(exact, got, 0), np.where(exact, want, 0).astype(np.int32))
            assert d is None, f"{what} [{fam.name}]: {d}"
    if "acc_planted" in g and "acc_hid" in stages:
        d = first_difference("acc_hid (planted rows)", t["acc_hid"][1][:, :g["acc_planted"].shape[1]], g["acc_planted"])
        assert d is None, f"{what} [{fam.name}]: {d}"
    if "probs" in stages:
        err = compare_rows(fam, g, t["probs"], what, probs_bar)
    return err


def compare_rows(fam, g, p, what, bar, key="probs", zeros=True, row_sums=True):
    """Soft-max rows `p` against the recorded ones: NaN positions, exact zeros (`zeros`: a device whose exp flushes where
    glibc's returns a denormal is held to them only where the reference's zeros come from an infinite total), |p - recorded|
    <= bar -> the largest error."""
    if fam.sample and key == "probs":
        assert np.array_equal(np.argwhere(np.isnan(p)), g["probs_nan"]), f"{what} [{fam.name}]: probs: NaN positions differ"
        assert not zeros or np.array_equal(np.argwhere(p == 0), g["probs_zero"]), f"{what} [{fam.name}]: probs: positions of exact 0 differ"
        if row_sums:  # another libm's expf moves every term, the total and so every entry by a few u RELATIVELY: the sum by a few u
            sums = p.astype(np.float64).sum(axis=1)
            assert np.allclose(sums, g["probs_row_sum"], rtol=0, atol=bar, equal_nan=True), f"{what} [{fam.name}]: probs: row sums differ"
        got, want = p[..., g["probs_cols"]], g["probs_sample"]
    else:
        got, want = p, g[key]
        nan_d = first_difference(key + " NaN positions", np.isnan(got), np.isnan(want))
        assert nan_d is None, f"{what} [{fam.name}]: {nan_d}"
        zero_d = first_difference(key + " exact zeros", got == 0, want == 0) if zeros else None
        assert zero_d is None, f"{what} [{fam.name}]: {zero_d}"
    with np.errstate(invalid="ignore"):
        diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    diff[np.isnan(got) & np.isnan(want)] = 0.0
    err = float(diff.max()) if diff.size else 0.0
    if not err <= bar:
        i = tuple(int(v) for v in np.argwhere(~(diff <= bar))[0])
        raise AssertionError(f"{what} [{fam.name}]: {key} frame {i[0]} node {i[1]}: got {got[i]!r} want {want[i]!r}, |d| {diff[i]:.3e} > {bar}")
    return err


def relative_ok(fam, g, p, what, c_e, key="probs", m=None):
    """softmax_ref.check of rows `p` against the float64 soft-max of the RECORDED logits (masked-out nodes: z = 0) -> the share
    of entries below 2^-126.  For the families whose rows the absolute bar cannot see (Family.rel)."""
    z = g["logits"] if m is None else np.where(m != 0, g["logits"], np.float32(0.0)).astype(np.float32)
    return SR.check(np.asarray(p), z, SR.rows_pad_of(z.shape[1]), f"{what} [{fam.name}] {key}", oracle_nan=np.isnan(g[key]), c_e=c_e)


# ---------------------------------------------------------------------------------------------------------------- properties
def int8_weights(path, fam, quantize):
    """The int8 weights of every int8 layer, through `quantize(w, cutoff) -> (wq, mult)` (whose bytes the fixture's wq_sha256
    pins) -> list of int8 [N][K]."""
    net = _F().read_model_bin(path)
    return [quantize(L.weights, fam.cutoff)[0] for L in net.layers[1:]]


def planted_events(g, wq):
    """Per int8 layer, the number of (frame, node) whose recorded accumulator tap differs from np.float32 of the unsaturated
    int32 dot product of the recorded u8 inputs and the int8 weights: the pmaddubsw events that reached the reference's
    numbers.  g: a fixture or the reference's taps (u8_acts, acc_hid, acc_out)."""
    counts = []
    nh = g["u8_acts"].shape[0]
    for j in range(nh):
        acc = g["acc_hid"][j] if j < nh - 1 else g["acc_out"]
        plain = np.rint(g["u8_acts"][j].astype(np.float64) @ wq[j].astype(np.float64).T)   # exact: |sum| <= K * 255 * 128 < 2^53
        counts.append(int((acc != plain.astype(np.float32)).sum()))
    return counts


def properties(fam, g, wq=None, plain_l0=None, base=None):
    """The conditions under which the family's fixture is not blind, asserted on the RECORDED data `g` alone -> the figures
    (a dict) that DESIGN.md quotes.  wq: the int8 weights (events); plain_l0: the plain build's l0_lin (fma); base: the
    cut-off-3 fixture of the same net (cutoff)."""
    import limit_nets as LN

    out = {}
    for prop in fam.props:
        if prop == "events":
            out["events"] = [int(v) for v in g["events"]]
            if not fam.sample:  # (a sampled family keeps hashes: its counts are the generator's, from the full arrays)
                assert planted_events(g, wq) == out["events"], f"{fam.name}: recorded event counts {out['events']} are not the data's"
            assert all(c > 0 for c in out["events"]), f"{fam.name}: an int8 layer without a saturation event in the recorded data: {out['events']}"
        elif prop == "extreme":
            assert float(g["acc_max"]) >= EXACT and int(g["acc_big"]) > 0, f"{fam.name}: no accumulator tap at or beyond 2^24"
            want = np.broadcast_to(np.float32(LN.planted_acc()), g["acc_planted"].shape)
            assert np.array_equal(g["acc_planted"].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), f"{fam.name}: planted rows"
            out["acc_max"], out["acc_big"] = float(g["acc_max"]), int(g["acc_big"])
        elif prop == "fma":
            share = float((_bits(g["l0_lin"]) != _bits(plain_l0)).mean())
            assert share >= 0.25, f"{fam.name}: only {share:.1%} of l0_lin differ between the FMA and the plain reference build"
            out["fma_share"] = share
        elif prop == "ovf":
            p = g["probs"]
            assert (np.isnan(p).sum(1) == 4).all() and (p[~np.isnan(p)] == 0).all(), f"{fam.name}: not four NaN and zeros in every row"
        elif prop == "tot":
            assert (g["probs"] == 0).all(), f"{fam.name}: not every entry is 0"
        elif prop == "und":
            p = g["probs"]
            share = float((p < SR.TINY).mean())
            assert share > 0 and not np.isnan(p).any(), f"{fam.name}: no probability below 2^-126"
            out["below_tiny"] = share
        elif prop == "normal":
            lo = float(g["probs_min"]) if fam.sample else float(g["probs"].min())
            nans = int(np.size(g["probs_nan"])) if fam.sample else int(np.isnan(g["probs"]).sum())
            assert lo >= SR.TINY and nans == 0, f"{fam.name}: a probability is not a normal fp32 (min {lo:.3e}, {nans} NaN)"
            out["probs_min"] = lo
        elif prop == "hostile":
            x, (_, planted, cleaned) = g["x"], hostile_features()
            assert np.isposinf(x[planted["inf"]]) and np.isneginf(x[planted["ninf"]]) and np.isnan(x[planted["nan"]])
            assert (x[planted["huge"][0]] == np.float32(3.0e38)).all()
            moved = {}
            for name, (row, _) in planted.items():
                moved[name] = int((g["u8_acts"][0][row] != g["u8_acts"][0][cleaned[name]]).sum())
                assert moved[name] > 0, f"{fam.name}: the {name} row has the bytes of the same row without it"
            out["hostile_bytes_moved"] = moved
        elif prop == "lazy":
            lz, O = g["lazy"], g["lazy"].shape[1]
            assert (lz[0] == np.float32(1.0) / np.float32(O)).all(), f"{fam.name}: the all-off row is not the constant 1/O"
            assert (lz[1, :-1] == lz[1, 0]).all() and lz[1, -1] != lz[1, 0], f"{fam.name}: the one-node row has no single differing entry"
            off = g["masks"] == 0
            for f in range(3, lz.shape[0]):
                assert np.unique(lz[f][off[f]]).size == 1, f"{fam.name}: masked-out entries of row {f} are not one value"
        elif prop == "signal":  # tests/signal_nets.py's condition on the last hidden layer of the recorded rows
            import signal_nets as SN

            frames, med, values = (float(v) for v in g["signal"])
            if not fam.sample:  # (a sampled family keeps hashes: its figures are the generator's, from the full layer)
                assert LN.signal_stats(g["u8_acts"][-1]) == (frames, med, values), f"{fam.name}: the recorded signal figures are not the data's"
            assert frames == int(g["rows"]) and values >= SN.MIN_VALUES and med >= SN.MIN_RANGE, \
                f"{fam.name}: {frames} distinct rows of {int(g['rows'])}, {values} byte values, median node range {med} at the last hidden layer"
            out["signal"] = [frames, med, values]
        elif prop == "cutoff":
            assert (g["mult"] != base["mult"]).all() and (g["wq_sha256"] != base["wq_sha256"]).all(), \
                f"{fam.name}: multipliers or quantized weights are the cut-off-3 ones"
            out["mult"] = [float(v) for v in g["mult"]]
    return out
