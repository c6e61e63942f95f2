"""The pair-saturation walk of every kernel that has one, with events on lone frames (tests/sat_switch.py).

The reference saturates every adjacent pair to int16 (pmaddubsw, dnn.cc:337-340); the library screens the listed pairs -- one
frame per lane, a ballot -- and corrects exactly where a lane fires.  The Gaussian fixtures of the other tests never fire that
walk (n256 / mid) or fire the same ~23 entries on every frame (full); the hot nets fire in nearly every frame.  Here each of
8 switches is on in exactly ONE frame of the batch, so every listed entry has its event on one frame of one tile: a screen
that misses one frame position (the odd-NF tail, a row clamp, the row swizzle, a stale next-k, a read from the wrong ring
buffer) changes a byte.  The lone frames sit on the in-tile rows 0, 31, 32 (MFMA block edge), Wf - 1, Wf (wave edge), T - 32,
T - 1 of a first, a middle and the last (partial) tile and on the batch's last frame; T and Wf come from the case table.  A
second batch per case turns a random switch on in half of the frames.

Every case runs under the launch recorder and asserts that the instance it names ran; everything is compared with the oracle
(never with another library path) on the planted frames, their neighbours and 64 random frames -- after asserting, from a
numpy replay of the oracle's activations, that the events in that sample are exactly the planted ones."""
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np
import pytest

import sat_switch as SS
from dispatch_ledger import _masked_out_ok, _softmax_ok, _softmax_rel_ok, launched
from fast_dnn_amd import api
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

HALF_ROWS = (0, 63, 64, 127, 128, 159, 160)  # the role-split kernels: rows of a 160-frame half, and the other half's first


@dataclass
class Case:
    id: str
    kind: str              # sat_switch.NETS, or tdiv.w252
    n: int
    T: int                 # frame tile of the instance under test
    Wf: int                # frames per wave along the tile: 32 * NF
    entry: str             # prod | taps | hidden | ppo | set
    must: tuple
    fuse: int = 0
    chain: tuple = (0, 0)  # one launch per hidden layer unless the case is about the chained kernel
    pp: tuple = (-1, 0)
    ppo: int = -1
    rows: tuple = None
    integer_only: bool = False


def _out(shape, width, fuse):
    """Names of the output instances of `shape` a dense and a masked pass of this width launch (launch_cfg, fdnn_gemm.hip)."""
    if fuse:
        a = "" if width % 32 == 0 else "_anyw"
        return (f"gemm.out.{shape}.fused{a}", f"gemm.out.{shape}.fused_masked{a}")
    return (f"gemm.out.{shape}." + ("plain" if width % 32 == 0 else "anyw"), f"gemm.out.{shape}." + ("masked" if width % 4 == 0 else "masked_anyw"))


CASES = []
# -- production instances, 256-wide nets: (n, T, Wf, hidden instance, output shape, widths)
for n, T, Wf, hid, shape, widths in (
        (33, 32, 32, "small.hid.nt32.prod", None, (252,)),
        (545, 32, 32, "small.hid.nt32.prod", "ft32", (252,)),
        (1300, 32, 32, "small.hid.nt64.prod", "ft32", (251,)),
        (1409, 32, 32, "gemm.hid.ft32.w1.prod", "ft32", (256,)),
        (6177, 32, 32, "gemm.hid.ft32.prod", "ft32", (252,)),
        (8257, 64, 64, "gemm.hid.ft64.prod", "ft64", (256, 251)),
        (16513, 128, 64, "gemm.hid.ft128.nt128.prod", "ft128.bk128", (256, 251)),   # (the output shape's wave spans the tile: Wf = T)
        (33025, 256, 128, "gemm.hid.ft256.prod", "ft256", (256, 252)),
        (65601, 320, 160, "gemm.hid.ft320.prod", "ft320", (256, 251))):
    for w in widths:
        outs = ("small.out.prod", "small.out.masked") if shape is None else _out(shape, w, 0)
        CASES.append(Case(f"prod.n{n}.w{w}", f"k256.w{w}", n, T, Wf, "prod", (hid,) + outs))
        if T >= 128:
            CASES.append(Case(f"fused.n{n}.w{w}", f"k256.w{w}", n, T, Wf, "prod", (hid,) + _out(shape, w, 1), fuse=1))
# -- the tap instances of the same shapes
for n, T, Wf, must in ((33, 32, 32, ("small.hid.nt32.tap", "small.out.tap")), (1300, 32, 32, ("small.hid.nt64.tap", "gemm.out.ft32.tap")),
                       (1409, 32, 32, ("gemm.hid.ft32.w1.tap",)), (6177, 32, 32, ("gemm.hid.ft32.tap",)),
                       (8257, 64, 64, ("gemm.hid.ft64.tap", "gemm.out.ft64.tap")),
                       (16513, 128, 64, ("gemm.hid.ft128.nt128.tap", "gemm.out.ft128.tap")),  # (the output shape here steps 64 bytes)
                       (33025, 256, 128, ("gemm.hid.ft256.tap", "gemm.out.ft256.tap")), (65601, 320, 160, ("gemm.hid.ft320.tap", "gemm.out.ft320.tap"))):
    CASES.append(Case(f"taps.n{n}", "k256.w252", n, T, Wf, "taps", must))
# -- the true-divide instances (one shape: 128 frames, one wave along them, 64-byte steps): a layer with listed pairs reaches them
#    through a bias that fails the bounded-|lin| clause of the division check (sat_switch.true_divide_net)
CASES.append(Case("tdiv.taps.n300", "tdiv.w252", 300, 128, 128, "taps", ("gemm.hid.tdiv.tap", "gemm.out.tdiv.tap"), integer_only=True))
CASES.append(Case("tdiv.prod.n300", "tdiv.w252", 300, 128, 128, "prod", ("gemm.hid.tdiv.prod", "gemm.out.tdiv.anyw", "gemm.out.tdiv.masked"), integer_only=True))
# -- K = 2048, two int8 hidden layers: a task of layer 2 follows a task of layer 1 in one workgroup of the chained kernel
#    (chain_frame_tile, fdnn_select.hpp: 1281 frames go as 320-frame tiles, 641 as 256-frame tiles)
CASES.append(Case("chain320.n1281", "k2048", 1281, 320, 160, "hidden", ("chain.ft320.fix",), chain=(1, 1)))
CASES.append(Case("chain256.n641", "k2048", 641, 256, 128, "hidden", ("chain.ft256.fix",), chain=(1, 1)))
for n in (641, 961):
    CASES.append(Case(f"pp.n{n}", "k2048", n, 320, 160, "hidden", ("pp.hid.fix",), pp=(1, 1), rows=HALF_ROWS))
    CASES.append(Case(f"ppo.n{n}", "k2048", n, 320, 160, "ppo", ("ppo.out.fix",), fuse=-1, ppo=1, rows=HALF_ROWS))
# -- the shared-node-set and the list kernels (32-frame tiles)
for n in (33, 100):
    CASES.append(Case(f"set.n{n}", "k256.w252", n, 32, 32, "set", ()))


# ------------------------------------------------------------------------------------------------------------ fixtures
_MODELS = {}


@pytest.fixture(scope="module")
def models(tmp_models):
    def get(kind):
        if kind not in _MODELS:
            path, plan = SS.model_file(tmp_models, kind)
            orc = Oracle(path)
            _MODELS[kind] = dict(path=path, plan=plan, dnn=api.QuantizedDnn.loadFromFile(path, device=0), orc=orc,
                                 wq=[orc.layer_wq(li) for li in range(1, orc.n_layers)])
        return _MODELS[kind]

    yield get
    for m in _MODELS.values():
        m["dnn"].delete()
        m["orc"].close()
    _MODELS.clear()


@pytest.fixture()
def modes():
    yield
    api.set_fuse(-1)
    api.set_chain(-1)
    api.set_pp(-1)
    api.set_ppo(-1)
    api.set_kernel(0)


def sample(n, frames, seed):
    """The rows the oracle scores: the given frames, their two neighbours and 64 further frames."""
    pick = {g for f in frames for g in (f - 1, f, f + 1) if 0 <= g < n}
    rng = np.random.default_rng(seed)
    target = min(n, len(pick) + 64)
    while len(pick) < target:
        pick.add(int(rng.integers(0, n)))
    return np.array(sorted(pick))


def taps_mt(orc, xs):
    """Oracle.calculate(taps=True) over frame ranges in parallel (frames are independent) -> (probs, taps)."""
    ch = Oracle._chunks(len(xs), Oracle.default_threads())
    with ThreadPoolExecutor(len(ch)) as ex:
        parts = list(ex.map(lambda r: orc.calculate(xs[r[0]:r[1]], taps=True), ch))
    wt = {k: np.concatenate([t[k] for _, t in parts], axis=1 if k in ("u8_acts", "acc_hid") else 0) for k in ("u8_acts", "acc_hid", "acc_out", "logits")}
    wt["sat_events"] = sum(t["sat_events"] for _, t in parts)
    return np.concatenate([w for w, _ in parts]), wt


def batches(case):
    """-> [(name, x, switches_on, idx)]: the lone-frame batch and the crowded one, with the rows the oracle scores."""
    frames = SS.lone_frames(case.n, case.T, case.Wf, rows=case.rows, seed=case.n)
    idx = sample(case.n, frames, seed=case.n)
    lone = SS.lone_switches(case.n, frames)
    crowd = SS.crowded_switches(case.n, seed=case.n + 1)
    base = SS.features(case.n, lone, seed=2000 + case.n % 977)
    xc = base.copy()
    xc[:, SS.SWITCH_COL:SS.SWITCH_COL + SS.S] = crowd
    return [("lone", base, lone, idx), ("crowded", xc, crowd, idx)]


def reference(m, x, on, idx, what):
    """The oracle on rows idx, after asserting that its events there are the planted ones: every entry of a switch on the
    frame that switch is on in, nothing else (a lone frame carries every entry of its switch, in every int8 layer)."""
    orc, plan = m["orc"], m["plan"]
    want, wt = taps_mt(orc, x[idx])
    total = 0
    for li in range(1, orc.n_layers):
        ev, acc = SS.pair_events(m["wq"][li - 1], wt["u8_acts"][li - 1])
        planted = plan.planted(li, on[idx])
        assert np.array_equal(SS.event_keys(ev), planted), f"{what}: layer {li}: the oracle's events are not the planted ones"
        assert np.array_equal(acc, wt["acc_out"] if li == orc.n_layers - 1 else wt["acc_hid"][li - 1])
        total += len(ev) if li < orc.n_layers - 1 else 0
    assert wt["sat_events"] == total and total > 0
    return want, wt


def probe_masks(m, n, seed):
    """Random byte masks, twice: every probe node of the output layer kept active, and every one masked out."""
    O = m["orc"].out_dim
    nodes = np.unique(m["plan"].entries(m["orc"].n_layers - 1)[:, 0])
    keep = np.random.default_rng(seed).integers(0, 2, size=(n, O), dtype=np.int8)
    drop = keep.copy()
    keep[:, nodes] = 1
    drop[:, nodes] = 0
    return keep, drop


def hidden_bytes(dnn, x):
    ctx = dnn.getNewLazyContext(x.shape[0])
    ctx.calculateUntilOutput(x)
    got = ctx.hiddenActivations().copy()
    ctx.delete()
    return got


def device_pass(dnn, x):
    import torch

    n = x.shape[0]
    xd = torch.from_numpy(x).cuda()
    out = torch.full((n, dnn.outputDimension()), float("nan"), dtype=torch.float32, device="cuda")
    dnn.calculate_device(xd.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# --------------------------------------------------------------------------------------------------------------- entries
def run_prod(case, m, x, idx, want, wt, what):
    dnn, orc = m["dnn"], m["orc"]
    keep, drop = probe_masks(m, case.n, seed=case.n)

    def go():
        hid = hidden_bytes(dnn, x)
        dense = dnn.productionOutputAcc(x, 1, probs=True)
        return hid, dense, [dnn.productionOutputAcc(x, 1, masks=mk, probs=True) for mk in (keep, drop)]

    (hid, (acc, dense), masked), ran = launched(go)
    assert set(case.must) <= ran, f"{what}: {sorted(set(case.must) - ran)} did not run; launched {sorted(ran)}"
    assert np.array_equal(hid[idx], wt["u8_acts"][-1]), f"{what}: last hidden layer's bytes differ from the oracle"
    assert np.array_equal(acc[idx], wt["acc_out"]), f"{what}: output accumulators differ from the oracle"
    if not case.integer_only:
        _softmax_rel_ok(dense[idx], want, orc, wt["acc_out"], what + " dense", tap=wt["logits"])
    for (macc, lazy), mk, tag in zip(masked, (keep, drop), ("probes active", "probes masked out")):
        on = mk[idx] != 0
        assert np.array_equal(macc[idx][on], wt["acc_out"][on]), f"{what}, {tag}: masked output accumulators differ from the oracle"
        if not case.integer_only:
            want_lazy = orc.output_mt(wt["u8_acts"][-1], masks=mk[idx])
            _softmax_rel_ok(lazy[idx], want_lazy, orc, wt["acc_out"], f"{what}, {tag}", masks=mk[idx])
            _masked_out_ok(lazy[idx], mk[idx], what)


def run_taps(case, m, x, idx, want, wt, what):
    got, ran = launched(m["dnn"].forwardTaps, x)
    assert set(case.must) <= ran, f"{what}: {sorted(set(case.must) - ran)} did not run; launched {sorted(ran)}"
    assert np.array_equal(got["acc_hid"][:, idx], wt["acc_hid"]), f"{what}: hidden accumulators differ from the oracle"
    assert np.array_equal(got["u8_acts"][:, idx], wt["u8_acts"]), f"{what}: hidden bytes differ from the oracle"
    assert np.array_equal(got["acc_out"][idx], wt["acc_out"]), f"{what}: output accumulators differ from the oracle"


def run_hidden(case, m, x, idx, want, wt, what):
    got, ran = launched(hidden_bytes, m["dnn"], x)
    assert set(case.must) <= ran, f"{what}: {sorted(set(case.must) - ran)} did not run; launched {sorted(ran)}"
    assert np.array_equal(got[idx], wt["u8_acts"][-1]), f"{what}: last hidden layer's bytes differ from the oracle"


def run_ppo(case, m, x, idx, want, wt, what):
    """The role-split output kernel serves the dense device call only -- the accumulator probe excludes it (choose_layer) -- so
    its walk is held to the probabilities: a dropped correction moves a logit by 0.28 or more.  The accumulators of the same
    batch come from the in-phase tiles the probe takes."""
    dnn, orc = m["dnn"], m["orc"]
    got, ran = launched(device_pass, dnn, x)
    assert set(case.must) <= ran, f"{what}: {sorted(set(case.must) - ran)} did not run; launched {sorted(ran)}"
    _softmax_ok(got[idx], want, what)
    _softmax_rel_ok(got[idx], want, orc, wt["acc_out"], what, tap=wt["logits"])
    acc, probs = dnn.productionOutputAcc(x, 1, probs=True)
    assert np.array_equal(acc[idx], wt["acc_out"]), f"{what}: output accumulators differ from the oracle"
    _softmax_rel_ok(probs[idx], want, orc, wt["acc_out"], what + " probe pass", tap=wt["logits"])


def run_set(case, m, x, idx, want, wt, what):
    """fdnn_set.hip (MFMA kernel with the walk; the fallback to the list kernels) and fdnn_lists.hip (score with the walk):
    node sets / lists holding every probe node of the output layer, half of them, none."""
    dnn, O = m["dnn"], m["orc"].out_dim
    probes = np.unique(m["plan"].entries(m["orc"].n_layers - 1)[:, 0])
    others = np.setdiff1d(np.arange(O), probes)
    sets = {"all": np.sort(np.concatenate([probes, others[::3]])), "half": np.sort(np.concatenate([probes[::2], others[1::3]])), "none": others}
    ctx = dnn.getNewLazyContext(case.n)
    ctx.calculateUntilOutput(x)
    try:
        for tag, nodes in sets.items():
            nodes = nodes.astype(np.int32)
            ref = wt["acc_out"][:, nodes]
            for mode in (1, 2):
                api.set_kernel(mode)
                sb, lb = api.set_launches(), api.lists_launches()
                acc = ctx.setAccumulators(nodes)
                sa, la = api.set_launches(), api.lists_launches()
                assert (sa[1] > sb[1] and sa[2] == sb[2]) if mode == 1 else (sa[2] > sb[2] and la[1] > lb[1]), (what, tag, mode, sb, sa, lb, la)
                assert np.array_equal(acc[idx], ref), f"{what}: set kernel mode {mode}, {tag} probe nodes: accumulators differ from the oracle"
            lb = api.lists_launches()
            rp = np.arange(case.n + 1, dtype=np.int32) * nodes.size
            acc = ctx.listsAccumulators(rp, np.tile(nodes, case.n)).reshape(case.n, nodes.size)
            assert api.lists_launches()[1] > lb[1]
            assert np.array_equal(acc[idx], ref), f"{what}: list kernel, {tag} probe nodes: accumulators differ from the oracle"
    finally:
        ctx.delete()


_RUN = {"prod": run_prod, "taps": run_taps, "hidden": run_hidden, "ppo": run_ppo, "set": run_set}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_lone_frame_events(case, models, modes):
    m = models(case.kind)
    api.set_fuse(case.fuse)
    api.set_chain(*case.chain)
    api.set_pp(*case.pp)
    api.set_ppo(case.ppo)
    for name, x, on, idx in batches(case):
        what = f"{case.id} ({name})"
        want, wt = reference(m, x, on, idx, what)
        _RUN[case.entry](case, m, x, idx, want, wt, what)
