"""The dispatch ledger: which kernel instance every case must launch, and the oracle parity each case is held to.

The library names every host launch branch (fdnn_note.hpp; api.launch_names()).  This module is the one table that says
which case covers which names:

  * CASES      every case names a net, a batch size, an entry point, the process-wide modes it sets, the names it exists
               for (`must`) and -- in EXPECT -- the exact set of names its recorded span launches;
  * EXCLUDED   names no case launches, each with the reason: ablation-only (the flag in the library's table), or
               unreachable in the shipped build, with the file and lines that show it.  (155 names: 33 ablation-only,
               4 excluded, 118 launched by the cases.)

tests/test_dispatch_ledger_host.py (no GPU) asserts  union(EXPECT) | EXCLUDED == the library's table,  so a new launch
branch without a case fails everywhere; tests/test_gpu_dispatch_ledger.py runs every case with the recorder on and
asserts the launched set in both directions plus parity with the oracle (never with another library path):
u8 activations and int32 accumulators bit-exact, tap logits bit-exact, soft-max <= 2e-6 absolute with the oracle's NaN
pattern AND within tests/softmax_ref.py's relative bound of exp(z - max) / sum in float64, masked-out entries one value per row.  Weight scales stay <= 0.05 wherever the soft-max is compared (the range tools/fuzz_parity.py
established 2e-6 for); the every-pair-saturating and degenerate nets are compared on integer state only.

Run as a script (`python tests/dispatch_ledger.py --run ID [ID ...]`) it runs cases in this process and prints one JSON
line per case: that is how cases that need an environment variable read at library load (FDNN_L0_TN) run in a child."""
import json
import os
import sys
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:  # (run as a script from another directory)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import softmax_ref as SR  # noqa: E402

TIGHT = 2e-6  # |p - oracle| per element: the project's soft-max bar (tests/test_gpu_production_shapes.py, tools/fuzz_parity.py)


# ---------------------------------------------------------------------------------------------------------------- nets
def _net(kind):
    """kind -> FloatNet.  'n256/W/mode', 'mid', 'full/mode', 'tdiv/W', 'allsat', 'wide/W' (2048 inputs), 'd64' (64 inputs), 'k2304', 'wout/W'."""
    from fast_dnn_amd import formats as F

    parts = kind.split("/")
    if parts[0] == "n256":  # one node tile in every layer: hidden and output layers select the same frame tile
        return F.synth_net([432, 256, 256, 256, int(parts[1])], seed=300 + int(parts[1]), mode=parts[2])
    if parts[0] == "mid":
        return F.synth_net([432, 256, 256, 256, 1000], seed=5)
    if parts[0] == "full":
        return F.synth_net(F.NET_TOPOLOGY, seed=1, mode=parts[1])
    if parts[0] == "tdiv":  # an all-zero int8 layer has multiplier round(127 / 0) = inf: the IEEE-divide instances
        net = F.synth_net([432, 128, 128, 128, int(parts[1])], seed=12)
        net.layers[2].weights[:] = 0.0
        net.layers[3].weights[:] = 0.0
        return net
    if parts[0] == "allsat":  # tests/test_gpu_production_shapes.py::test_net_with_every_pair_saturating
        net = F.synth_net([432, 256, 256, 256, 300], seed=17)
        rng = np.random.default_rng(5)
        for L in net.layers[1:]:
            L.weights[:] = rng.choice(np.array([-0.5, 0.5, 0.45, -0.48], np.float32), size=L.weights.shape)
        return net
    if parts[0] == "wide":
        return F.synth_net([2048, 256, 256, 256, 64], seed=21, w0_std=0.01)
    if parts[0] == "k2304":  # rows longer than the small-batch kernels take (K > 2048): the tiled shapes from one frame up
        return F.synth_net([432, 2304, 2304, 2304, 252], seed=61)
    if parts[0] == "wout":  # an output layer of 129 node tiles behind rows too long for the small-batch kernel: one frame tile of
        # every output shape is a launch of its own here, and frame_tile's cost model (fdnn_select.hpp) prefers the 128-frame tiles (321 .. 384 frames)
        return F.synth_net([432, 2304, 2304, 2304, int(parts[1])], seed=71)
    if parts[0] == "d64":
        return F.synth_net([64, 256, 256, 256, 252], seed=41)
    # -- the soft-max range nets (tests/softmax_ref.py, tests/test_gpu_softmax_range.py): a net of the ledger with other output
    #    biases -- the bias is added after the division, so the logits move and nothing upstream of them does
    if parts[0] in ("lad", "ladfull"):  # 'lad/W', 'ladfull': a shuffled ladder over [-40, 20]: exp's argument over 87 units, every probability a normal fp32
        net = _net(f"n256/{parts[1]}/gauss" if parts[0] == "lad" else "full/gauss")
        net.layers[-1].bias = SR.ladder(net.layers[-1].bias.size, -40.0, 20.0, seed=net.layers[-1].bias.size)
        return net
    if parts[0] in ("tail", "tailfull"):  # 'tail/ovf|tot|und', 'tailfull/ovf': the ends of exp's range.  Output weights / 256 (a power of
        # two: the same int8 weights, a 256 times larger multiplier) leave |acc / coef| below 0.05, so the logits are the biases to that
        net = _net("n256/256/gauss" if parts[0] == "tail" else "full/gauss")
        out = net.layers[-1]
        out.weights = (out.weights / np.float32(256.0)).astype(np.float32)
        W = out.bias.size
        rng = np.random.default_rng(W + len(parts[1]))
        if parts[1] == "ovf":    # four logits at 95: exp is +inf (from 88.73), the total +inf, those four NaN and every other entry 0
            out.bias = SR.ladder(W, -40.0, 20.0, seed=W + 1)
            out.bias[rng.choice(W, 4, replace=False)] = 95.0
        elif parts[1] == "tot":  # 64 logits at 87: every exp finite (6e37), the row total +inf, every entry 0
            out.bias = SR.ladder(W, -40.0, 20.0, seed=W + 2)
            out.bias[rng.choice(W, 64, replace=False)] = 87.0
        elif parts[1] == "und":  # a ladder over [-120, 0]: probabilities below 2^-126 beside normal ones
            out.bias = SR.ladder(W, -120.0, 0.0, seed=W + 3)
        else:
            raise ValueError(kind)
        return net
    raise ValueError(kind)


def net_path(kind, cache_dir=None):
    from fast_dnn_amd import formats as F

    d = cache_dir or os.environ.get("TMPDIR", "/tmp")
    if kind.startswith("full/"):
        p = os.path.join(d, f"fdnn_net_seed1_{kind.split('/')[1]}.bin")
        return F.ensure_model_file(p, F.NET_TOPOLOGY, seed=1, mode=kind.split("/")[1])
    p = os.path.join(d, "fdnn_ledger_" + kind.replace("/", "_") + ".bin")
    net = _net(kind)
    if not (os.path.exists(p) and os.path.getsize(p) == F.model_bin_size([net.layers[0].weights.shape[1]] + [L.weights.shape[0] for L in net.layers])):
        tmp = f"{p}.tmp{os.getpid()}"
        F.write_model_bin(tmp, net)
        os.replace(tmp, p)
    return p


# --------------------------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    id: str
    net: str
    n: int
    entry: str             # taps | prod | dense_device | dense_host | lazy_bytes | lazy_bits | onecall_bytes | onecall_bits |
    #                        server | server_lazy | raw | l0 | l0_probe | load | blob
    must: tuple            # the names this case exists for (a subset of EXPECT[id])
    fuse: int = 1          # fdnn_debug_set_fuse: 1 fused soft-max wherever the shape allows, 0 the scale pass
    chain: tuple = (-1, 0) # fdnn_debug_set_chain
    pp: tuple = (-1, 0)    # fdnn_debug_set_pp
    ppo: int = -1          # fdnn_debug_set_ppo
    l0_kernel: int = 0     # fdnn_debug_set_l0_kernel
    fma: bool = False      # setInputLayerFma (the oracle follows)
    tile: int = 0          # frame tile of the instance under test: where the row sample of a K = 2048 case is centred
    integer_only: bool = False  # nets outside the soft-max bar's range: integer state only
    env: dict = field(default_factory=dict)  # read at library load: the case runs in a child process


CASES = []


def _add(*a, **k):
    c = Case(*a, **k)
    if c.net.startswith("n256/") and c.entry == "prod":
        # one launch per hidden layer: from ~9 800 frames the default rule would chain these 256-wide layers (K % 128 == 0),
        # and the per-layer shapes' edges are what these cases are for; the chained kernel has its own cases below
        c.chain = (0, 0)
    CASES.append(c)


def _w(i):  # output widths by edge index: rows % 32 == 0, rows % 4 == 0 only, rows % 4 != 0
    return (256, 252, 251)[i % 3]


# -- one node tile per layer: hidden and output layer of a batch take the same frame tile.  n = 0, 1, T - 1 (mod T).
#    unfused soft-max: plain / anyw / masked / masked_anyw per tile; hidden: small -> ft32.w1 -> ft32 -> ft64 -> nt128 -> ft256 -> ft320
for i, n in enumerate((544, 545, 575)):
    _add(f"n256.small_ft32.n{n}", f"n256/{_w(i)}/gauss", n, "prod", ("small.hid.nt32.prod", "gemm.out.ft32." + ("plain", "anyw", "anyw")[i],
                                                                   "gemm.out.ft32." + ("masked", "masked", "masked_anyw")[i]), fuse=0)
for i, n in enumerate((1408, 1409, 1439)):
    _add(f"n256.w1.n{n}", f"n256/{_w(i)}/gauss", n, "prod", ("gemm.hid.ft32.w1.prod",), fuse=0)
for i, n in enumerate((6176, 6177, 6207)):
    _add(f"n256.ft32.n{n}", f"n256/{_w(i)}/gauss", n, "prod", ("gemm.hid.ft32.prod", "gemm.out.ft32." + ("plain", "anyw", "anyw")[i]), fuse=0)
for i, n in enumerate((8256, 8257, 8319)):
    _add(f"n256.ft64.n{n}", f"n256/{_w(i)}/gauss", n, "prod", ("gemm.hid.ft64.prod", "gemm.out.ft64." + ("plain", "anyw", "anyw")[i],
                                                              "gemm.out.ft64." + ("masked", "masked", "masked_anyw")[i]), fuse=0)
for i, n in enumerate((16512, 16513, 16639)):
    _add(f"n256.ft128.unfused.n{n}", f"n256/{_w(i)}/gauss", n, "prod", ("gemm.hid.ft128.nt128.prod", "gemm.out.ft128.bk128." + ("plain", "anyw", "anyw")[i],
                                                                       "gemm.out.ft128.bk128." + ("masked", "masked", "masked_anyw")[i]), fuse=0)
    _add(f"n256.ft128.fused.n{n}", f"n256/{_w(i)}/gauss", n, "prod", ("gemm.out.ft128.bk128." + ("fused", "fused_anyw", "fused_anyw")[i],
                                                                     "gemm.out.ft128.bk128." + ("fused_masked", "fused_masked_anyw", "fused_masked_anyw")[i]))
for T, sizes in ((256, (33024, 33025, 33279)), (320, (65600, 65601, 65919))):
    for i, n in enumerate(sizes):
        _add(f"n256.ft{T}.unfused.n{n}", f"n256/{_w(i)}/gauss", n, "prod", (f"gemm.hid.ft{T}.prod", f"gemm.out.ft{T}." + ("plain", "anyw", "anyw")[i],
                                                                           f"gemm.out.ft{T}." + ("masked", "masked", "masked_anyw")[i]), fuse=0)
        mode = ("gauss", "nosat", "gauss")[i]  # the walk-free instances: pair-free layers, widths that are multiples of 32
        w = (256, 256, 251)[i]
        _add(f"n256.ft{T}.fused.n{n}", f"n256/{w}/{mode}", n, "prod",
             ((f"gemm.hid.ft{T}.prod", f"gemm.out.ft{T}.fused", f"gemm.out.ft{T}.fused_masked"),
              (f"gemm.hid.ft{T}.prod_nofix", f"gemm.out.ft{T}.fused_nofix", f"gemm.out.ft{T}.fused_masked_nofix"),
              (f"gemm.hid.ft{T}.prod", f"gemm.out.ft{T}.fused_anyw", f"gemm.out.ft{T}.fused_masked_anyw"))[i])
# a single tile of the small-batch kernels and their 32-frame edges; 64-node tiles of the small hidden kernel
for i, n in enumerate((1, 31, 32, 33, 512)):
    _add(f"n256.small.n{n}", f"n256/{_w(i)}/gauss", n, "prod", ("small.hid.nt32.prod", "small.out.prod", "small.out.masked"), fuse=0)
# a single tile of the tiled shapes: only layers too long for the small-batch kernels reach them below 513 frames
for n in (1, 32):
    _add(f"k2304.single_tile.n{n}", "k2304", n, "prod", ("gemm.hid.ft32.w1.prod", "gemm.out.ft32.anyw", "gemm.out.ft32.masked"), fuse=0)
# a wide output layer (129 node tiles, K = 2304): single-tile launches of the 64-, 128- (128-byte-step), 256- and 320-frame output
# shapes, and the 64-byte-step 128-frame shape, which the cost model picks where three 128-frame tiles per node tile fit one
# round of 512 and two 256-frame tiles need two rounds of 256 (321 .. 384 frames; n = 1 mod 128 is outside that window).
# Its own single tile needs more than 256 node tiles (an output layer of 65 537 nodes or more, a 570 MB model): not built here.
# Hidden layers are at most 128 node tiles wide (fdnn_model.cpp:346) and reach one frame tile only of ft32.w1 (the k2304 cases):
# one tile of ft32 needs more than 192 node tiles (launch_qgemm `case 32`), of ft64 / ft128.bk128 / ft256 / ft320 at least 129
# (below, a batch that fits one such tile fits one round of smaller ones), of the 128 x 128 shape more than 32 768 padded rows.
for n, w, shape in ((33, 33021, "ft64"), (64, 33024, "ft64"), (65, 33021, "ft128.bk128"), (128, 33024, "ft128.bk128"), (129, 33021, "ft256"),
                    (256, 33024, "ft256"), (257, 33021, "ft320"), (320, 33024, "ft320"), (321, 33024, "ft128"), (383, 33021, "ft128"), (384, 33024, "ft128")):
    _add(f"wout.{shape}.n{n}", f"wout/{w}", n, "prod", tuple(f"gemm.out.{shape}.{b}" for b in (("plain", "masked") if w % 32 == 0 else ("anyw", "masked_anyw"))), fuse=0)
_add("n256.small_nt64.n1300", "n256/252/gauss", 1300, "prod", ("small.hid.nt64.prod",), fuse=0)
# -- the tap instances of every shape
for n, must in ((33, ("small.hid.nt32.tap", "small.out.tap", "l0.small.tap")), (300, ("l0.tile16.tap",)), (1000, ("l0.tile32.tap",)),
                (1300, ("small.hid.nt64.tap", "gemm.out.ft32.tap")),
                (1409, ("gemm.hid.ft32.w1.tap",)), (6177, ("gemm.hid.ft32.tap",)), (8257, ("gemm.hid.ft64.tap", "gemm.out.ft64.tap")),
                (16513, ("gemm.hid.ft128.nt128.tap", "gemm.out.ft128.tap")), (33025, ("gemm.hid.ft256.tap", "gemm.out.ft256.tap")),
                (65601, ("gemm.hid.ft320.tap", "gemm.out.ft320.tap"))):
    _add(f"n256.taps.n{n}", "n256/252/gauss", n, "taps", must)
# -- the true-divide shape (one frame tile: 128)
_add("tdiv.taps.n129", "tdiv/252", 129, "taps", ("gemm.hid.tdiv.tap", "gemm.out.tdiv.tap"), integer_only=True)
_add("tdiv.prod.n128", "tdiv/256", 128, "prod", ("gemm.hid.tdiv.prod", "gemm.out.tdiv.plain", "gemm.out.tdiv.masked"), integer_only=True)
_add("tdiv.prod.n127", "tdiv/251", 127, "prod", ("gemm.hid.tdiv.prod", "gemm.out.tdiv.anyw", "gemm.out.tdiv.masked_anyw"), integer_only=True)
_add("tdiv.prod.n1", "tdiv/252", 1, "prod", ("gemm.hid.tdiv.prod", "gemm.out.tdiv.anyw", "gemm.out.tdiv.masked"), integer_only=True)
# -- every pair saturating: the entry walk of the small-batch and of the tiled instances, integer state
_add("allsat.taps.n700", "allsat", 700, "taps", ("small.hid.nt32.tap",), integer_only=True)
_add("allsat.prod.n700", "allsat", 700, "prod", ("small.hid.nt32.prod",), integer_only=True, fuse=0)
_add("allsat.prod.n1409", "allsat", 1409, "prod", ("gemm.hid.ft32.w1.prod",), integer_only=True, fuse=0)
# -- layer 0
_add("l0.small.n100", "mid", 100, "l0", ("l0.small.prod",))
_add("l0.tile16.n300", "mid", 300, "l0", ("l0.tile16.prod",), l0_kernel=2)
_add("l0.tile32.n1000", "mid", 1000, "l0", ("l0.tile32.prod",), l0_kernel=2)
_add("l0.tile64.n1201", "mid", 1201, "l0", ("l0.tile64.prod",), l0_kernel=2)
_add("l0.tile64.taps.n1201", "mid", 1201, "taps", ("l0.tile64.tap",), l0_kernel=2)
_add("l0.chain12.n700", "mid", 700, "l0", ("l0.chain.jc12.tn64.prod", "l0.image.frames"), l0_kernel=1)
_add("l0.chain12.taps.n700", "mid", 700, "taps", ("l0.chain.jc12.tn64.tap",), l0_kernel=1)
_add("l0.chain16.n700", "d64", 700, "l0", ("l0.chain.jc16.tn64.prod",), l0_kernel=1)
_add("l0.chain16.taps.n700", "d64", 700, "taps", ("l0.chain.jc16.tn64.tap",), l0_kernel=1)
for kind, tag in (("mid", "12"), ("d64", "16")):
    _add(f"l0.chain{tag}.tn128.n700", kind, 700, "l0", (f"l0.chain.jc{tag}.tn128.prod",), l0_kernel=1, env={"FDNN_L0_TN": "128"})
    _add(f"l0.chain{tag}.tn128.taps.n700", kind, 700, "taps", (f"l0.chain.jc{tag}.tn128.tap",), l0_kernel=1, env={"FDNN_L0_TN": "128"})
_add("l0.split64.n600", "mid", 600, "l0", ("l0.digits", "l0.split.n64", "l0.fixlist.lpo8"))
_add("l0.split128.n2999", "full/gauss", 2999, "l0", ("l0.split.n128", "l0.fixlist.lpo8"))
_add("l0.split128.n3000", "full/gauss", 3000, "l0", ("l0.split.n128", "l0.fixlist.lpo4"))
_add("l0.screen.n2048", "mid", 2048, "l0", ("l0.screen.f128", "l0.fix.tiles"), l0_kernel=3)
_add("l0.probe.n300", "mid", 300, "l0_probe", ("l0.split.n128.probe",))
_add("l0.mfma.n300", "mid", 300, "l0", ("l0.mfma.prod",), fma=True)
_add("l0.mfma.taps.n300", "mid", 300, "taps", ("l0.mfma.tap",), fma=True)
# -- K = 2048: the chained hidden layers, the role-split kernels (sampled rows; frames are independent)
for n in (10239, 10240, 10241):
    _add(f"full.chain320.n{n}", "full/gauss", n, "lazy_bytes", ("chain.ft320.fix",), chain=(1, 1), tile=320)
for n in (9728, 9983):
    _add(f"full.chain256.n{n}", "full/gauss", n, "lazy_bytes", ("chain.ft256.fix",), chain=(1, 1), tile=256)
_add("full.chain256.nofix.default.n12000", "full/nosat", 12000, "lazy_bytes", ("chain.ft256.nofix",), tile=256)
_add("full.chain320.nofix.n10240", "full/nosat", 10240, "lazy_bytes", ("chain.ft320.nofix",), chain=(1, 1), tile=320)
_add("full.chain256.nofix.n9728", "full/nosat", 9728, "lazy_bytes", ("chain.ft256.nofix",), chain=(1, 1), tile=256)
for n in (16640, 16641, 16959):
    _add(f"full.pp.nofix.n{n}", "full/nosat", n, "lazy_bytes", ("pp.hid.nofix",), chain=(0, 0), tile=320)
_add("full.pp.nofix.default.n20480", "full/nosat", 20480, "lazy_bytes", ("pp.hid.nofix",), tile=320)
_add("full.pp.fix.n6401", "full/gauss", 6401, "lazy_bytes", ("pp.hid.fix",), chain=(0, 0), pp=(1, 1), tile=320)
for n in (513, 640, 641):
    _add(f"full.ppo.fix.n{n}", "full/gauss", n, "dense_device", ("ppo.out.fix",), ppo=1, tile=320)
_add("full.ppo.fix.default.n7040", "full/gauss", 7040, "dense_device", ("ppo.out.fix",), tile=320)
_add("full.ppo.nofix.default.n4480", "full/nosat", 4480, "dense_device", ("ppo.out.nofix",), tile=320)
_add("full.fused320.n10000", "full/gauss", 10000, "prod", ("gemm.hid.ft320.prod", "gemm.out.ft320.fused", "gemm.out.ft320.fused_masked"), chain=(0, 0), tile=320)
# -- the other entry points
_add("entry.dense_host.n300", "mid", 300, "dense_host", ("norm.small",), fuse=0)
_add("entry.dense_host.n25000", "n256/252/gauss", 25000, "dense_host", ("norm.rows",), fuse=0)
_add("entry.dense_device.n1025", "n256/251/gauss", 1025, "dense_device", ("norm.rows",), fuse=0)
_add("entry.lazy_bytes.n300", "mid", 300, "lazy_bytes", ("small.out.masked", "compact"))
_add("entry.lazy_bytes.n8256", "n256/256/gauss", 8256, "lazy_bytes", ("maskpack.flat", "compact"))
_add("entry.lazy_bytes.n8257", "n256/251/gauss", 8257, "lazy_bytes", ("maskpack.rows", "compact"))
_add("entry.lazy_bits.n300", "mid", 300, "lazy_bits", ("maskunpack", "compact"))
_add("entry.lazy_bits.n8257", "n256/251/gauss", 8257, "lazy_bits", ("gemm.out.ft64.masked_anyw", "compact"))
_add("entry.onecall_bytes.n300", "mid", 300, "onecall_bytes", ("small.out.masked",))
_add("entry.onecall_bits.n300", "mid", 300, "onecall_bits", ("maskunpack",))
_add("entry.server.n300", "mid", 300, "server", ("small.out.prod", "norm.small"), fuse=0)
_add("entry.server_lazy.n300", "mid", 300, "server_lazy", ("compact",))
_add("entry.raw.n300", "mid", 300, "raw", ("splice",))
# -- model load
_add("load.file", "mid", 0, "load", ("fastdiv_check", "l0.image.weights"))
_add("load.blob", "mid", 0, "blob", ("l0.image.weights",))

# The exact set of names every case's recorded span launches (the GPU test asserts it in both directions).
EXPECT = {
    "n256.small_ft32.n544": {"gemm.out.ft32.masked", "gemm.out.ft32.plain", "l0.tile32.prod", "maskpack.flat", "norm.small", "small.hid.nt32.prod"},
    "n256.small_ft32.n545": {"gemm.out.ft32.anyw", "gemm.out.ft32.masked", "l0.tile32.prod", "maskpack.rows", "norm.small", "small.hid.nt32.prod"},
    "n256.small_ft32.n575": {
        "gemm.out.ft32.anyw", "gemm.out.ft32.masked_anyw", "l0.digits", "l0.fixlist.lpo8", "l0.split.n64", "maskpack.rows", "norm.rows",
        "small.hid.nt32.prod"},
    "n256.w1.n1408": {
        "gemm.hid.ft32.w1.prod", "gemm.out.ft32.masked", "gemm.out.ft32.plain", "l0.digits", "l0.fixlist.lpo8", "l0.split.n64", "maskpack.flat",
        "norm.rows"},
    "n256.w1.n1409": {
        "gemm.hid.ft32.w1.prod", "gemm.out.ft32.anyw", "gemm.out.ft32.masked", "l0.digits", "l0.fixlist.lpo8", "l0.split.n64", "maskpack.rows",
        "norm.rows"},
    "n256.w1.n1439": {
        "gemm.hid.ft32.w1.prod", "gemm.out.ft32.anyw", "gemm.out.ft32.masked_anyw", "l0.digits", "l0.fixlist.lpo8", "l0.split.n64", "maskpack.rows",
        "norm.rows"},
    "n256.ft32.n6176": {
        "gemm.hid.ft32.prod", "gemm.out.ft32.masked", "gemm.out.ft32.plain", "l0.digits", "l0.fixlist.lpo4", "l0.split.n64", "maskpack.flat",
        "norm.rows"},
    "n256.ft32.n6177": {
        "gemm.hid.ft32.prod", "gemm.out.ft32.anyw", "gemm.out.ft32.masked", "l0.digits", "l0.fixlist.lpo4", "l0.split.n64", "maskpack.rows",
        "norm.rows"},
    "n256.ft32.n6207": {
        "gemm.hid.ft32.prod", "gemm.out.ft32.anyw", "gemm.out.ft32.masked_anyw", "l0.digits", "l0.fixlist.lpo4", "l0.split.n64", "maskpack.rows",
        "norm.rows"},
    "n256.ft64.n8256": {
        "gemm.hid.ft64.prod", "gemm.out.ft64.masked", "gemm.out.ft64.plain", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat",
        "norm.rows"},
    "n256.ft64.n8257": {
        "gemm.hid.ft64.prod", "gemm.out.ft64.anyw", "gemm.out.ft64.masked", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.rows",
        "norm.rows"},
    "n256.ft64.n8319": {
        "gemm.hid.ft64.prod", "gemm.out.ft64.anyw", "gemm.out.ft64.masked_anyw", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.rows",
        "norm.rows"},
    "n256.ft128.unfused.n16512": {
        "gemm.hid.ft128.nt128.prod", "gemm.out.ft128.bk128.masked", "gemm.out.ft128.bk128.plain", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128",
        "maskpack.flat", "norm.rows"},
    "n256.ft128.fused.n16512": {
        "gemm.hid.ft128.nt128.prod", "gemm.out.ft128.bk128.fused", "gemm.out.ft128.bk128.fused_masked", "l0.digits", "l0.fixlist.lpo4",
        "l0.split.n128", "maskpack.flat"},
    "n256.ft128.unfused.n16513": {
        "gemm.hid.ft128.nt128.prod", "gemm.out.ft128.bk128.anyw", "gemm.out.ft128.bk128.masked", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128",
        "maskpack.rows", "norm.rows"},
    "n256.ft128.fused.n16513": {
        "gemm.hid.ft128.nt128.prod", "gemm.out.ft128.bk128.fused_anyw", "gemm.out.ft128.bk128.fused_masked_anyw", "l0.digits", "l0.fixlist.lpo4",
        "l0.split.n128", "maskpack.rows"},
    "n256.ft128.unfused.n16639": {
        "gemm.hid.ft128.nt128.prod", "gemm.out.ft128.bk128.anyw", "gemm.out.ft128.bk128.masked_anyw", "l0.digits", "l0.fixlist.lpo4",
        "l0.split.n128", "maskpack.rows", "norm.rows"},
    "n256.ft128.fused.n16639": {
        "gemm.hid.ft128.nt128.prod", "gemm.out.ft128.bk128.fused_anyw", "gemm.out.ft128.bk128.fused_masked_anyw", "l0.digits", "l0.fixlist.lpo4",
        "l0.split.n128", "maskpack.rows"},
    "n256.ft256.unfused.n33024": {
        "gemm.hid.ft256.prod", "gemm.out.ft256.masked", "gemm.out.ft256.plain", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat",
        "norm.rows"},
    "n256.ft256.fused.n33024": {
        "gemm.hid.ft256.prod", "gemm.out.ft256.fused", "gemm.out.ft256.fused_masked", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128",
        "maskpack.flat"},
    "n256.ft256.unfused.n33025": {
        "gemm.hid.ft256.prod", "gemm.out.ft256.anyw", "gemm.out.ft256.masked", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.rows",
        "norm.rows"},
    "n256.ft256.fused.n33025": {
        "gemm.hid.ft256.prod_nofix", "gemm.out.ft256.fused_masked_nofix", "gemm.out.ft256.fused_nofix", "l0.digits", "l0.fixlist.lpo4",
        "l0.split.n128", "maskpack.flat"},
    "n256.ft256.unfused.n33279": {
        "gemm.hid.ft256.prod", "gemm.out.ft256.anyw", "gemm.out.ft256.masked_anyw", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128",
        "maskpack.rows", "norm.rows"},
    "n256.ft256.fused.n33279": {
        "gemm.hid.ft256.prod", "gemm.out.ft256.fused_anyw", "gemm.out.ft256.fused_masked_anyw", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128",
        "maskpack.rows"},
    "n256.ft320.unfused.n65600": {
        "gemm.hid.ft320.prod", "gemm.out.ft320.masked", "gemm.out.ft320.plain", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat",
        "norm.rows"},
    "n256.ft320.fused.n65600": {
        "gemm.hid.ft320.prod", "gemm.out.ft320.fused", "gemm.out.ft320.fused_masked", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128",
        "maskpack.flat"},
    "n256.ft320.unfused.n65601": {
        "gemm.hid.ft320.prod", "gemm.out.ft320.anyw", "gemm.out.ft320.masked", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.rows",
        "norm.rows"},
    "n256.ft320.fused.n65601": {
        "gemm.hid.ft320.prod_nofix", "gemm.out.ft320.fused_masked_nofix", "gemm.out.ft320.fused_nofix", "l0.digits", "l0.fixlist.lpo4",
        "l0.split.n128", "maskpack.flat"},
    "n256.ft320.unfused.n65919": {
        "gemm.hid.ft320.prod", "gemm.out.ft320.anyw", "gemm.out.ft320.masked_anyw", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128",
        "maskpack.rows", "norm.rows"},
    "n256.ft320.fused.n65919": {
        "gemm.hid.ft320.prod", "gemm.out.ft320.fused_anyw", "gemm.out.ft320.fused_masked_anyw", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128",
        "maskpack.rows"},
    "n256.small.n1": {"l0.small.prod", "norm.small", "small.hid.nt32.prod", "small.out.masked", "small.out.prod"},
    "n256.small.n31": {"l0.small.prod", "norm.small", "small.hid.nt32.prod", "small.out.masked", "small.out.prod"},
    "n256.small.n32": {"l0.small.prod", "norm.rows", "small.hid.nt32.prod", "small.out.masked", "small.out.prod"},
    "n256.small.n33": {"l0.small.prod", "norm.small", "small.hid.nt32.prod", "small.out.masked", "small.out.prod"},
    "n256.small.n512": {"l0.tile32.prod", "norm.small", "small.hid.nt32.prod", "small.out.masked", "small.out.prod"},
    "k2304.single_tile.n1": {"gemm.hid.ft32.w1.prod", "gemm.out.ft32.anyw", "gemm.out.ft32.masked", "l0.small.prod", "maskpack.rows", "norm.small"},
    "k2304.single_tile.n32": {"gemm.hid.ft32.w1.prod", "gemm.out.ft32.anyw", "gemm.out.ft32.masked", "l0.small.prod", "maskpack.rows", "norm.small"},
    "wout.ft64.n33": {"gemm.hid.ft32.w1.prod", "gemm.out.ft64.anyw", "gemm.out.ft64.masked_anyw", "l0.small.prod", "maskpack.rows", "norm.rows"},
    "wout.ft64.n64": {"gemm.hid.ft32.w1.prod", "gemm.out.ft64.masked", "gemm.out.ft64.plain", "l0.small.prod", "maskpack.flat", "norm.rows"},
    "wout.ft128.bk128.n65": {"gemm.hid.ft32.w1.prod", "gemm.out.ft128.bk128.anyw", "gemm.out.ft128.bk128.masked_anyw", "l0.small.prod", "maskpack.rows", "norm.rows"},
    "wout.ft128.bk128.n128": {"gemm.hid.ft32.w1.prod", "gemm.out.ft128.bk128.masked", "gemm.out.ft128.bk128.plain", "l0.small.prod", "maskpack.flat", "norm.rows"},
    "wout.ft256.n129": {"gemm.hid.ft32.w1.prod", "gemm.out.ft256.anyw", "gemm.out.ft256.masked_anyw", "l0.tile16.prod", "maskpack.rows", "norm.rows"},
    "wout.ft256.n256": {"gemm.hid.ft32.w1.prod", "gemm.out.ft256.masked", "gemm.out.ft256.plain", "l0.tile16.prod", "maskpack.flat", "norm.rows"},
    "wout.ft320.n257": {"gemm.hid.ft32.w1.prod", "gemm.out.ft320.anyw", "gemm.out.ft320.masked_anyw", "l0.tile16.prod", "maskpack.rows", "norm.rows"},
    "wout.ft320.n320": {"gemm.hid.ft32.w1.prod", "gemm.out.ft320.masked", "gemm.out.ft320.plain", "l0.tile16.prod", "maskpack.flat", "norm.rows"},
    "wout.ft128.n321": {"gemm.hid.ft32.w1.prod", "gemm.out.ft128.masked", "gemm.out.ft128.plain", "l0.tile32.prod", "maskpack.flat", "norm.rows"},
    "wout.ft128.n383": {"gemm.hid.ft32.w1.prod", "gemm.out.ft128.anyw", "gemm.out.ft128.masked_anyw", "l0.tile32.prod", "maskpack.rows", "norm.rows"},
    "wout.ft128.n384": {"gemm.hid.ft32.w1.prod", "gemm.out.ft128.masked", "gemm.out.ft128.plain", "l0.tile32.prod", "maskpack.flat", "norm.rows"},
    "n256.small_nt64.n1300": {
        "gemm.out.ft32.anyw", "gemm.out.ft32.masked", "l0.digits", "l0.fixlist.lpo8", "l0.split.n64", "maskpack.rows", "norm.rows",
        "small.hid.nt64.prod"},
    "n256.taps.n33": {"l0.small.tap", "norm.small", "small.hid.nt32.tap", "small.out.tap", "xor80"},
    "n256.taps.n300": {"l0.tile16.tap", "norm.small", "small.hid.nt32.tap", "small.out.tap", "xor80"},
    "n256.taps.n1000": {"gemm.out.ft32.tap", "l0.tile32.tap", "norm.small", "small.hid.nt32.tap", "xor80"},
    "n256.taps.n1300": {"gemm.out.ft32.tap", "l0.tile64.tap", "norm.rows", "small.hid.nt64.tap", "xor80"},
    "n256.taps.n1409": {"gemm.hid.ft32.w1.tap", "gemm.out.ft32.tap", "l0.tile64.tap", "norm.rows", "xor80"},
    "n256.taps.n6177": {"gemm.hid.ft32.tap", "gemm.out.ft32.tap", "l0.tile64.tap", "norm.rows", "xor80"},
    "n256.taps.n8257": {"gemm.hid.ft64.tap", "gemm.out.ft64.tap", "l0.tile64.tap", "norm.rows", "xor80"},
    "n256.taps.n16513": {"gemm.hid.ft128.nt128.tap", "gemm.out.ft128.tap", "l0.tile64.tap", "norm.rows", "xor80"},
    "n256.taps.n33025": {"gemm.hid.ft256.tap", "gemm.out.ft256.tap", "l0.tile64.tap", "norm.rows", "xor80"},
    "n256.taps.n65601": {"gemm.hid.ft320.tap", "gemm.out.ft320.tap", "l0.chain.jc12.tn64.tap", "l0.image.frames", "norm.rows", "xor80"},
    "tdiv.taps.n129": {"gemm.hid.tdiv.tap", "gemm.out.tdiv.tap", "l0.tile16.tap", "norm.small", "small.hid.nt32.tap", "xor80"},
    "tdiv.prod.n128": {
        "gemm.hid.tdiv.prod", "gemm.out.tdiv.masked", "gemm.out.tdiv.plain", "l0.small.prod", "maskpack.flat", "norm.small", "small.hid.nt32.prod"},
    "tdiv.prod.n127": {
        "gemm.hid.tdiv.prod", "gemm.out.tdiv.anyw", "gemm.out.tdiv.masked_anyw", "l0.small.prod", "maskpack.rows", "norm.rows",
        "small.hid.nt32.prod"},
    "tdiv.prod.n1": {
        "gemm.hid.tdiv.prod", "gemm.out.tdiv.anyw", "gemm.out.tdiv.masked", "l0.small.prod", "maskpack.rows", "norm.small", "small.hid.nt32.prod"},
    "allsat.taps.n700": {"gemm.out.ft32.tap", "l0.tile32.tap", "norm.small", "small.hid.nt32.tap", "xor80"},
    "allsat.prod.n700": {
        "gemm.out.ft32.anyw", "gemm.out.ft32.masked", "l0.digits", "l0.fixlist.lpo8", "l0.split.n64", "maskpack.rows", "norm.small",
        "small.hid.nt32.prod"},
    "allsat.prod.n1409": {
        "gemm.hid.ft32.w1.prod", "gemm.out.ft32.anyw", "gemm.out.ft32.masked", "l0.digits", "l0.fixlist.lpo8", "l0.split.n64", "maskpack.rows",
        "norm.rows"},
    "l0.small.n100": {"l0.small.prod"},
    "l0.tile16.n300": {"l0.tile16.prod"},
    "l0.tile32.n1000": {"l0.tile32.prod"},
    "l0.tile64.n1201": {"l0.tile64.prod"},
    "l0.tile64.taps.n1201": {"gemm.out.ft32.tap", "l0.tile64.tap", "norm.rows", "small.hid.nt32.tap", "xor80"},
    "l0.chain12.n700": {"l0.chain.jc12.tn64.prod", "l0.image.frames"},
    "l0.chain12.taps.n700": {"gemm.out.ft32.tap", "l0.chain.jc12.tn64.tap", "l0.image.frames", "norm.small", "small.hid.nt32.tap", "xor80"},
    "l0.chain16.n700": {"l0.chain.jc16.tn64.prod", "l0.image.frames"},
    "l0.chain16.taps.n700": {"gemm.out.ft32.tap", "l0.chain.jc16.tn64.tap", "l0.image.frames", "norm.small", "small.hid.nt32.tap", "xor80"},
    "l0.chain12.tn128.n700": {"l0.chain.jc12.tn128.prod", "l0.image.frames"},
    "l0.chain12.tn128.taps.n700": {"gemm.out.ft32.tap", "l0.chain.jc12.tn128.tap", "l0.image.frames", "norm.small", "small.hid.nt32.tap", "xor80"},
    "l0.chain16.tn128.n700": {"l0.chain.jc16.tn128.prod", "l0.image.frames"},
    "l0.chain16.tn128.taps.n700": {"gemm.out.ft32.tap", "l0.chain.jc16.tn128.tap", "l0.image.frames", "norm.small", "small.hid.nt32.tap", "xor80"},
    "l0.split64.n600": {"l0.digits", "l0.fixlist.lpo8", "l0.split.n64"},
    "l0.split128.n2999": {"l0.digits", "l0.fixlist.lpo8", "l0.split.n128"},
    "l0.split128.n3000": {"l0.digits", "l0.fixlist.lpo4", "l0.split.n128"},
    "l0.screen.n2048": {"l0.fix.tiles", "l0.screen.f128"},
    "l0.probe.n300": {"l0.digits", "l0.fixlist.lpo8", "l0.split.n128.probe"},
    "l0.mfma.n300": {"l0.mfma.prod"},
    "l0.mfma.taps.n300": {"l0.mfma.tap", "norm.small", "small.hid.nt32.tap", "small.out.tap", "xor80"},
    "full.chain320.n10239": {
        "chain.ft320.fix", "compact", "gemm.out.ft320.fused_masked", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat"},
    "full.chain320.n10240": {
        "chain.ft320.fix", "compact", "gemm.out.ft320.fused_masked", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat"},
    "full.chain320.n10241": {
        "chain.ft320.fix", "compact", "gemm.out.ft256.fused_masked", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat"},
    "full.chain256.n9728": {
        "chain.ft256.fix", "compact", "gemm.out.ft320.fused_masked", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat"},
    "full.chain256.n9983": {
        "chain.ft256.fix", "compact", "gemm.out.ft320.fused_masked", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat"},
    "full.chain256.nofix.default.n12000": {
        "chain.ft256.nofix", "compact", "gemm.out.ft256.fused_masked_nofix", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat"},
    "full.chain320.nofix.n10240": {
        "chain.ft320.nofix", "compact", "gemm.out.ft320.fused_masked_nofix", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat"},
    "full.chain256.nofix.n9728": {
        "chain.ft256.nofix", "compact", "gemm.out.ft320.fused_masked_nofix", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat"},
    "full.pp.nofix.n16640": {
        "compact", "gemm.out.ft320.fused_masked_nofix", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat", "pp.hid.nofix"},
    "full.pp.nofix.n16641": {
        "compact", "gemm.out.ft320.fused_masked_nofix", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat", "pp.hid.nofix"},
    "full.pp.nofix.n16959": {
        "compact", "gemm.out.ft320.fused_masked_nofix", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat", "pp.hid.nofix"},
    "full.pp.nofix.default.n20480": {
        "compact", "gemm.out.ft320.fused_masked_nofix", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat", "pp.hid.nofix"},
    "full.pp.fix.n6401": {"compact", "gemm.out.ft320.fused_masked", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat", "pp.hid.fix"},
    "full.ppo.fix.n513": {"l0.tile32.prod", "ppo.out.fix", "small.hid.nt64.prod"},
    "full.ppo.fix.n640": {"l0.digits", "l0.fixlist.lpo8", "l0.split.n64", "ppo.out.fix", "small.hid.nt64.prod"},
    "full.ppo.fix.n641": {"l0.digits", "l0.fixlist.lpo8", "l0.split.n64", "ppo.out.fix", "small.hid.nt64.prod"},
    "full.ppo.fix.default.n7040": {"gemm.hid.ft256.prod", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "ppo.out.fix"},
    "full.ppo.nofix.default.n4480": {"gemm.hid.ft256.prod_nofix", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "ppo.out.nofix"},
    "full.fused320.n10000": {
        "gemm.hid.ft320.prod", "gemm.out.ft320.fused", "gemm.out.ft320.fused_masked", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128",
        "maskpack.flat"},
    "entry.dense_host.n300": {"l0.tile16.prod", "norm.small", "small.hid.nt32.prod", "small.out.prod"},
    "entry.dense_host.n25000": {"chain.ft256.fix", "gemm.out.ft128.bk128.anyw", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "norm.rows"},
    "entry.dense_device.n1025": {"gemm.out.ft32.anyw", "l0.digits", "l0.fixlist.lpo8", "l0.split.n64", "norm.rows", "small.hid.nt32.prod"},
    "entry.lazy_bytes.n300": {"compact", "l0.tile16.prod", "maskpack.rows", "norm.small", "small.hid.nt32.prod", "small.out.masked"},
    "entry.lazy_bytes.n8256": {
        "compact", "gemm.hid.ft64.prod", "gemm.out.ft64.masked", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.flat", "norm.rows"},
    "entry.lazy_bytes.n8257": {
        "compact", "gemm.hid.ft64.prod", "gemm.out.ft64.masked_anyw", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "maskpack.rows", "norm.rows"},
    "entry.lazy_bits.n300": {"compact", "l0.tile16.prod", "maskunpack", "norm.small", "small.hid.nt32.prod", "small.out.masked"},
    "entry.lazy_bits.n8257": {
        "compact", "gemm.hid.ft64.prod", "gemm.out.ft64.masked_anyw", "l0.digits", "l0.fixlist.lpo4", "l0.split.n128", "norm.rows"},
    "entry.onecall_bytes.n300": {"compact", "l0.tile16.prod", "maskunpack", "norm.small", "small.hid.nt32.prod", "small.out.masked"},
    "entry.onecall_bits.n300": {"compact", "l0.tile16.prod", "maskunpack", "norm.small", "small.hid.nt32.prod", "small.out.masked"},
    "entry.server.n300": {"l0.tile16.prod", "norm.small", "small.hid.nt32.prod", "small.out.prod"},
    "entry.server_lazy.n300": {"compact", "l0.tile16.prod", "maskunpack", "norm.small", "small.hid.nt32.prod", "small.out.masked"},
    "entry.raw.n300": {"l0.tile16.prod", "norm.small", "small.hid.nt32.prod", "small.out.prod", "splice"},
    "load.file": {"fastdiv_check", "l0.image.weights"},
    "load.blob": {"l0.image.weights"},
}

# Names no case launches.  Ablation-only names (flag 1 in the library's table: the branch needs a -DFDNN_ABLATION build)
# are excluded by that flag; the names below are unreachable in the shipped build for the reason given.  The library compiles
# only the instances its table names (launch_cfg, fdnn_gemm.hip:1140-1163), and what no selection can reach has been deleted;
# what is left here is the hidden-layer side of the two four-wave 128-frame shapes, which gemm_shape's `case 128`
# (fdnn_select.hpp:200-203; launch_qgemm, fdnn_gemm.hip:1213-1214) keeps as the arms of a 256-node, 128-frame hidden launch --
# what a measurement build's forced FDNN_NODE_TILE=256 takes; without them the switch would need an error path.
# The argument: (a) frame_tile (fdnn_select.hpp:112-145) returns 128 either from its first loop (:122-123: where
# rows_pad / 256 * ceil(n / 128) <= 256) or from the cost model below it, and from the cost model only for layers of 129 node
# tiles or more (33 024 padded rows): tests/host/select_check.cpp (tests/test_select_host.py) evaluates the function itself for
# every width the loader accepts (fdnn_model.cpp:315, :374: 2^19 output nodes) up to the frame count beyond which the 128-frame
# tiles' 465 per 512 tiles can no longer undercut 320 per 256 tiles of 320 frames whatever the rounding; (b) hidden layers are at
# most 32 768 wide (fdnn_model.cpp:346, :374), 128 node tiles.  (The same statement keeps fused_ok's 128-frame clause,
# fdnn_select.hpp:217, from ever refusing a launch: a fused launch has at most 32 node tiles.)
_FT128_HID = ("fdnn_model.cpp:346 (hidden width <= 32 768 = 128 node tiles) and fdnn_select.hpp:122-144 (with fdnn_select.cpp: no forced tile in the shipped "
              "build): for such a layer frame tile 128 comes only from "
              "frame_tile's first loop, where rows_pad / 256 * ceil(n / 128) <= 256 < rows_pad / 256 * ceil(n / 64) puts rows_pad / 128 * ceil(n / 128) "
              "in (256, 512] and node_tile (:170-171, choose_layer :268-269) answers 128: the 2 x 2-wave shape (gemm.hid.ft128.nt128.*), taps included; "
              "the true-divide layers (also frame tile 128) take their own shape")
EXCLUDED = {
    "unlisted": "fdnn_gemm.hip:1140-1198 (launch_cfg) against fdnn_note.hpp FDNN_GEMM_LAUNCH_NAMES: every branch of the launcher names a listed (shape, branch); "
                "the catch-all counts a launch only if the table and the launcher disagree",
    **{f"gemm.hid.ft128.{b}": _FT128_HID for b in ("prod", "tap")},
    "gemm.hid.ft128.bk128.prod": _FT128_HID,
}


# -------------------------------------------------------------------------------------------------------------- runner
def launched(fn, *args, **kwargs):
    """fn(*args, **kwargs) with the recorder on -> (its result, the names of the kernel instances launched meanwhile).
    The tests that switch a mode and compare bytes use it to show that the mode they forced is what ran."""
    from fast_dnn_amd import api

    api.launch_record(True)
    api.launch_reset()
    try:
        res = fn(*args, **kwargs)
        return res, set(api.launch_counts())
    finally:
        api.launch_record(False)  # off is the library's default: the tests that follow run as a caller's process does


def chain_tile(n):
    """Frame tile of the chained hidden-layer kernel (chain_frame_tile, fdnn_select.hpp): 320 unless 256-frame tiles pad
    more than 64 frames less."""
    return 256 if (-n % 256) + 64 < (-n % 320) else 320


def sample_rows(n, tile, seed):
    """Rows a K = 2048 case lets the oracle score: row 0, row n - 1, the two rows either side of the multiples of `tile`
    nearest n / 2 and nearest n, and 64 further rows (fixed by seed)."""
    pick = {0, n - 1}
    for target in (n / 2, n):
        m = int(round(target / tile)) * tile
        for r in (m - 1, m):
            if 0 <= r < n:
                pick.add(r)
    rng = np.random.default_rng(seed)
    while len(pick) < min(n, 64 + 6):
        pick.add(int(rng.integers(0, n)))
    return np.array(sorted(pick))


def _softmax_ok(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs from the oracle"
    err = float(np.nanmax(np.abs(got - want))) if got.size else 0.0
    assert err <= TIGHT, f"{what}: soft-max differs from the oracle by {err:.3e} (> {TIGHT})"


def _softmax_rel_ok(got, want, orc, acc, what, masks=None, tap=None):
    """The relative bar beside the absolute one: against exp(z - max) / sum in float64 within softmax_ref.bound, z the
    reference's fp32 logits rebuilt from the oracle's accumulators (and equal, bit for bit, to its `logits` tap where there is one)."""
    z = SR.logits(acc, SR.coef_of(orc), orc.layer_bias(orc.n_layers - 1), masks=masks, tap=tap)
    share = SR.check(got, z, SR.rows_pad_of(orc.out_dim), what, oracle_nan=np.isnan(want))
    assert share == 0.0, f"{what}: {share:.3%} of the entries lie below 2^-126 and took check()'s weaker rule"


def _masked_out_ok(got, masks, what):
    """Masked-out nodes of a row all carry the row's 1 / total (exp(0) / total, dnn.cc:366-369): one value per row."""
    off = masks == 0
    lo = np.where(off, got, np.inf).min(1)
    hi = np.where(off, got, -np.inf).max(1)
    rows = off.any(1)
    assert np.array_equal(lo[rows], hi[rows]) and (lo[rows] > 0).all(), f"{what}: masked-out entries are not one value per row"


_MODELS = {}
LAST_COUNTS = {}   # launches per name of the latest run_case span in this process
LAST_AUDIT = {}    # the scratch audit of the latest run_case span (api.scratch_dirty()), a child's included
AUDIT_TOTAL = {"cases": 0, "contexts": 0, "seconds": 0.0}  # over every span judged in this process


class ScratchSpan:
    """The scratch audit over a span of calls on one model: every context that goes back to the pool or
    is destroyed inside the span -- the entry points' own, the pool's, a scoring loop's slots -- is counted, and close()
    asserts that none of them held a non-zero counter, that at least one was looked at, and that the model's fault counters
    stand where they stood.  `dnn` may be None (a span that loads its own model: pass it to close())."""

    def __init__(self, dnn=None):
        from fast_dnn_amd import api

        api.scratch_dirty()  # (totals of whatever ran before are not this span's)
        api.scratch_audit(True)
        self.before = self._counters(dnn) if dnn is not None else (0, 0, 0)

    @staticmethod
    def _counters(dnn):
        return dnn.chainFaults(), int(dnn.deviceCounters(4)[3]), dnn.fuseGiveups()

    @staticmethod
    def stop():
        """Ends the span without judging it -> the totals."""
        from fast_dnn_amd import api

        api.scratch_audit(False)
        return api.scratch_dirty()

    def close(self, what, dnn=None, min_contexts=1):
        after = self._counters(dnn) if dnn is not None else None
        check_audit(what, self.stop(), min_contexts)
        if after is not None:
            assert after[0] == self.before[0] and after[1] == self.before[1], \
                f"{what}: chained launches ran into their wait bound: chainFaults {self.before[0]} -> {after[0]}, device counter [3] {self.before[1]} -> {after[1]}"
            assert after[2] == self.before[2], f"{what}: fused soft-max tiles gave up waiting: fuseGiveups {self.before[2]} -> {after[2]}"


def check_audit(what, totals, min_contexts=1):
    from fast_dnn_amd import api

    LAST_AUDIT.clear()
    LAST_AUDIT.update(totals)
    AUDIT_TOTAL["cases"] += 1
    AUDIT_TOTAL["contexts"] += totals["contexts"]
    AUDIT_TOTAL["seconds"] += totals.get("seconds", 0.0)
    dirty = {k: totals[k] for k in api.scratch_names() if totals[k]}
    assert not dirty, f"{what}: scratch audit: counters left non-zero after their launch (buffer: words) {dirty} over {totals['contexts']} contexts"
    assert totals["unreadable"] == 0, f"{what}: scratch audit: {totals['unreadable']} contexts could not be read"
    assert totals["contexts"] >= min_contexts, f"{what}: scratch audit looked at {totals['contexts']} contexts (at least {min_contexts} expected): the check is blind"
CHILD_COUNTS = {}  # case id -> launches per name of a span that ran in a child process (the parent's recorder does not see them)


def _model(case):
    from fast_dnn_amd import api
    from oracle.oracle import Oracle

    if case.net not in _MODELS:
        p = net_path(case.net)
        _MODELS[case.net] = (p, api.QuantizedDnn.loadFromFile(p, device=0), Oracle(p))
    return _MODELS[case.net]


def release_models():
    for _, dnn, orc in _MODELS.values():
        dnn.delete()
        orc.close()
    _MODELS.clear()


def run_case(case, detail=None):
    """Run one case with the recorder on -> the set of names its span launched.  Raises AssertionError on a parity miss.
    A caller that adds checks of its own (tests/test_gpu_softmax_range.py) passes a dict as `detail` and finds there what the
    case produced and what the oracle says on the rows compared: got, idx, masks, orc and -- taps: want, wt; otherwise: hid,
    want, acc (the oracle's dense probabilities and output accumulators)."""
    import contextlib

    from fast_dnn_amd import api, formats as F
    from oracle.oracle import Oracle

    api.launch_record(True)
    if case.entry in ("load", "blob"):
        return _run_load(case)
    path, dnn, orc = _model(case)
    D, O = dnn.inputDimension(), dnn.outputDimension()
    n = case.n
    x = F.synth_features(n, D, seed=1000 + n % 977, pad_from=None if D != 432 else 429)
    big = "full" in case.net.split("/")[0]  # K = 2048, 8000 outputs: the oracle scores a sample of the rows
    idx = sample_rows(n, case.tile or 320, seed=n) if big else np.arange(n)
    soft = not case.integer_only
    api.set_fuse(case.fuse)
    api.set_chain(*case.chain)
    api.set_pp(*case.pp)
    api.set_ppo(case.ppo)
    dnn.setInputLayerKernel(case.l0_kernel)
    dnn.setInputLayerFma(case.fma)
    Oracle.set_l0_fma(case.fma)
    span = None
    try:
        gen = F.generate_masks_fast if n * O > (1 << 24) else F.generate_masks  # (same statistics; the per-frame Python loop costs seconds there)
        masks = gen(n, O, 0.40, 0.03, seed=7 + n % 89) if case.entry not in ("taps", "l0", "l0_probe", "dense_host", "dense_device", "server", "raw") else None
        span = ScratchSpan(dnn)
        api.launch_reset()
        got = _ENTRIES[case.entry](case, dnn, x, masks)
        LAST_COUNTS.clear()
        LAST_COUNTS.update(api.launch_counts())
        names = set(LAST_COUNTS)
        # ---- every context the span used left its counters as it found them (the entries delete or release theirs)
        closing, span = span, None
        closing.close(case.id, dnn)
        # ---- the oracle, on the rows the case compares
        xs = x[idx]
        if detail is not None:
            detail.update(got=got, idx=idx, masks=masks, orc=orc)
        if case.entry == "taps":
            want, wt = orc.calculate(xs, taps=True)
            if detail is not None:
                detail.update(want=want, wt=wt)
            for k in ("u8_acts", "acc_hid", "acc_out"):
                assert np.array_equal(got[k], wt[k]), f"{case.id}: {k} differs from the oracle"
            if soft:
                assert np.array_equal(got["logits"].view(np.uint32), wt["logits"].view(np.uint32)), f"{case.id}: logits differ from the oracle"
                _softmax_ok(got["probs"], want, case.id)
                _softmax_rel_ok(got["probs"], want, orc, wt["acc_out"], case.id, tap=wt["logits"])
            return names
        hid = orc.hidden_acts_mt(xs)
        if "hidden" in got:
            assert np.array_equal(got["hidden"][idx], hid), f"{case.id}: last hidden layer's bytes differ from the oracle"
        if "u8" in got:  # layer 0 alone
            _, wt = orc.calculate(xs, taps=True)
            assert np.array_equal(got["u8"][idx], wt["u8_acts"][0]), f"{case.id}: layer-0 bytes differ from the oracle"
        if "dense" in got or "acc" in got or "macc" in got or ("lazy" in got and soft) or detail is not None:
            want, acc = orc.output_mt(hid, want_acc=True)
            if detail is not None:
                detail.update(hid=hid, want=want, acc=acc)
            if "acc" in got:
                assert np.array_equal(got["acc"][idx], acc), f"{case.id}: output accumulators differ from the oracle"
            if "macc" in got:
                on = masks[idx] != 0
                assert np.array_equal(got["macc"][idx][on], acc[on]), f"{case.id}: masked output accumulators differ from the oracle"
            if "dense" in got and soft:
                _softmax_ok(got["dense"][idx], want, case.id + " dense")
                _softmax_rel_ok(got["dense"][idx], want, orc, acc, case.id + " dense")
        if "lazy" in got and soft:
            want_lazy = orc.output_mt(hid, masks=masks[idx])
            _softmax_ok(got["lazy"][idx], want_lazy, case.id + " lazy")
            _softmax_rel_ok(got["lazy"][idx], want_lazy, orc, acc, case.id + " lazy", masks=masks[idx])
            _masked_out_ok(got["lazy"][idx], masks[idx], case.id)
        return names
    finally:
        if span is not None:
            span.stop()
        api.set_fuse(-1)
        api.set_chain(-1)
        api.set_pp(-1)
        api.set_ppo(-1)
        dnn.setInputLayerKernel(0)
        dnn.setInputLayerFma(False)
        Oracle.set_l0_fma(False)


def _hidden(dnn, x):
    ctx = dnn.getNewLazyContext(x.shape[0])
    ctx.calculateUntilOutput(x)
    return ctx


def _e_taps(case, dnn, x, masks):
    return dnn.forwardTaps(x)


def _e_prod(case, dnn, x, masks):
    """The production instances under the accumulator probe, dense and masked, and the last hidden layer's bytes."""
    ctx = _hidden(dnn, x)
    out = {"hidden": ctx.hiddenActivations()}
    ctx.delete()
    out["acc"], out["dense"] = dnn.productionOutputAcc(x, 1, probs=True)
    out["macc"], out["lazy"] = dnn.productionOutputAcc(x, 1, masks=masks, probs=True)
    return out


def _e_dense_device(case, dnn, x, masks):
    import torch

    n = x.shape[0]
    ctx = _hidden(dnn, x)
    out = {"hidden": ctx.hiddenActivations()}
    ctx.delete()
    xd = torch.from_numpy(x).cuda()
    od = torch.full((n, dnn.outputDimension()), float("nan"), dtype=torch.float32, device="cuda")
    dnn.calculate_device(xd.data_ptr(), n, od.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out["dense"] = od.cpu().numpy()
    return out


def _e_dense_host(case, dnn, x, masks):
    return {"dense": dnn.calculate(x)}


def _e_lazy(case, dnn, x, masks):
    from fast_dnn_amd import formats as F

    ctx = _hidden(dnn, x)
    out = {"hidden": ctx.hiddenActivations()}
    if case.entry == "lazy_bits":
        out["lazy"] = ctx.calculateForOutputNodesBatchBits(F.pack_mask_bits(masks))
    else:
        out["lazy"] = ctx.calculateForOutputNodesBatch(masks)
    ctx.delete()
    return out


def _e_onecall(case, dnn, x, masks):
    from fast_dnn_amd import formats as F

    if case.entry == "onecall_bits":
        return {"lazy": dnn.calculateLazy(x, bits=F.pack_mask_bits(masks))}
    return {"lazy": dnn.calculateLazy(x, masks=masks)}


def _e_server(case, dnn, x, masks):
    from fast_dnn_amd import api, formats as F

    srv = api.ScoringServer(dnn, 512, 2)
    try:
        if case.entry == "server_lazy":
            t, out = srv.submitLazy(x, F.pack_mask_bits(masks))
        else:
            t, out = srv.submit(x)
        srv.wait(t)
    finally:
        srv.close()
    return {"lazy" if case.entry == "server_lazy" else "dense": out}


def _e_raw(case, dnn, x, masks):
    """Raw frames spliced on the device; the oracle scores the host-spliced rows (which replace x in place)."""
    from fast_dnn_amd import convert as CV

    offsets, raw_dim = list(range(-5, 6)), 39
    raw = np.ascontiguousarray(x[:, :raw_dim])
    dnn.setSplice(offsets, raw_dim)
    try:
        out = dnn.calculateRaw(raw)
    finally:
        dnn.setSplice([], 0)
    x[:] = CV.splice_frames(raw, offsets, x.shape[1])
    return {"dense": out}


def _e_l0(case, dnn, x, masks):
    u8, _ = dnn.layer0(x)
    return {"u8": u8}


def _e_l0_probe(case, dnn, x, masks):
    u8 = dnn.layer0Screen(x)[0]
    return {"u8": u8}


_ENTRIES = {"taps": _e_taps, "prod": _e_prod, "dense_device": _e_dense_device, "dense_host": _e_dense_host, "lazy_bytes": _e_lazy,
            "lazy_bits": _e_lazy, "onecall_bytes": _e_onecall, "onecall_bits": _e_onecall, "server": _e_server, "server_lazy": _e_server,
            "raw": _e_raw, "l0": _e_l0, "l0_probe": _e_l0_probe}


def _run_load(case):
    """The recorded span is the model load itself; what it produced is read back from the device: the blob's sections equal
    the host half's (tests/test_host_half.py pins those); the division verdict fastdiv_check wrote into the header lets this
    net's layers take the validated-division instances (no true-divide name runs in a tap pass, whose integers the oracle
    checks); and the layer-0 weight image it built feeds the chain kernel, whose bytes the oracle checks."""
    import struct

    import torch

    from fast_dnn_amd import api, formats as F
    from oracle.oracle import Oracle

    p = net_path(case.net)
    host = api.HostModel(p)
    want_blob = host.blob().copy()
    host.close()
    src = None
    span = ScratchSpan()  # (the load itself makes no context: the span runs on over the checks below, which make several)
    api.launch_reset()
    if case.entry == "blob":
        src = api.QuantizedDnn.loadFromFile(p, device=0)
        nbytes = src.blobSize()
        buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        src.exportBlob(buf.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        api.launch_reset()
        dnn = api.QuantizedDnn.fromDeviceBlob(buf.data_ptr(), nbytes, 0)
    else:
        dnn = api.QuantizedDnn.loadFromFile(p, device=0)
    LAST_COUNTS.clear()
    LAST_COUNTS.update(api.launch_counts())
    names = set(LAST_COUNTS)
    api.launch_record(False)  # the checks below launch kernels of their own
    try:
        nbytes = dnn.blobSize()
        out = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        dnn.exportBlob(out.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got_blob = out.cpu().numpy()
        assert got_blob.size == want_blob.size
        info = api.host_blob_check(got_blob)
        assert info == api.host_blob_check(want_blob)
        # the header is rewritten at load (the division verdicts); every section behind it is the host half's, byte for byte
        header_end = min(struct.unpack_from("<6Q", want_blob, 48))  # BlobHeader: the six section offsets follow 16 + 8 * 4 bytes; sections start behind it
        diff = np.flatnonzero(got_blob != want_blob)
        assert diff.size == 0 or diff.max() < header_end, f"{case.id}: device blob differs from the host half's at byte {diff.max()} (header ends at {header_end})"
        x = F.synth_features(700, dnn.inputDimension(), seed=5)
        dnn.setInputLayerKernel(1)  # the chain kernel reads the weight image built at load
        u8, _ = dnn.layer0(x)
        _, wt = Oracle(p).calculate(x, taps=True)
        assert np.array_equal(u8, wt["u8_acts"][0]), f"{case.id}: the layer-0 weight image built at load gives other bytes than the oracle"
        t, ran = launched(dnn.forwardTaps, x[:64])
        assert not any(".tdiv." in k for k in ran) and {"small.hid.nt32.tap", "small.out.tap"} <= ran, f"{case.id}: the load's division verdict sends this net to {sorted(ran)}"
        assert np.array_equal(t["acc_out"], wt["acc_out"][:64]) and np.array_equal(t["acc_hid"], wt["acc_hid"][:, :64])
        span.close(case.id, dnn)  # (a model of this span: its fault counters started at zero)
    finally:
        span.stop()
        api.launch_record(True)
        dnn.delete()
        if src is not None:
            src.delete()
    return names


def run_case_in_child(case, timeout=600):
    """Cases whose switch is read once at library load: a fresh interpreter with the case's environment."""
    import subprocess

    env = dict(os.environ, **case.env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--run", case.id], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["id"] == case.id and res["ok"], res
    CHILD_COUNTS[case.id] = {k: int(v) for k, v in res["counts"].items()}
    check_audit(case.id + " (child)", res["audit"])
    return set(res["names"])


def by_id(case_id):
    return next(c for c in CASES if c.id == case_id)


if __name__ == "__main__":
    if len(sys.argv) < 3 or sys.argv[1] != "--run":
        sys.exit("usage: dispatch_ledger.py --run CASE_ID [CASE_ID ...]")
    rc = 0
    for cid in sys.argv[2:]:
        try:
            got = run_case(by_id(cid))
            print(json.dumps({"id": cid, "ok": True, "names": sorted(got), "counts": dict(LAST_COUNTS), "audit": dict(LAST_AUDIT)}), flush=True)
        except AssertionError as e:
            print(json.dumps({"id": cid, "ok": False, "names": [], "counts": {}, "audit": dict(LAST_AUDIT), "error": str(e)}), flush=True)
            rc = 1
    release_models()
    sys.exit(rc)
