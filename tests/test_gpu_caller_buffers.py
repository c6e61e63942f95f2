"""The device-resident entry points on CALLER-OWNED buffers: what they write besides the result, what they read besides
the input, and whether they work where a caller's slice happens to start (tests/guarded.py).

Every case places all of a call's device buffers at once inside guarded allocations -- outputs between sentinel guards of a
whole 320-row tile of padded rows, inputs between poison (NaN around frames, 1 / -128 bytes around byte masks, all-ones
words around bit masks, negative indices around lists) -- and asserts
  (a) every guard and every input intact, no output element left unwritten;
  (b) the payload bit-identical to the same call on fresh, exactly sized, 256-byte-aligned buffers with CLEAN masks (rows do
      not depend on placement: fixed-order sums; a non-zero mask byte is a non-zero mask byte; bits past output_dim are ignored);
  (c) a row sample (rows 0, T - 1, T, n - 1 and 32 seeded rows) held to the oracle by the ledger's own checks,
and that the instance the case names ran (the launch recorder).  Nets, batch sizes and mode switches are the dispatch ledger's:
the smallest shapes at which each instance launches, with n = 1 (mod T) so that the last tile has one live row.

Base alignment (include/fdnn.h, "Device buffers"): element alignment for every buffer but the frames d_x of the quantized
net, which layer 0 reads by 16-byte LDS-DMA: those sit on 16-byte boundaries here (off the 256-byte grid all the same), and
test_frames_off_16_bytes_are_refused_before_any_launch holds the entry points to FDNN_E_ARG.  Float and int32 buffers run at
4, 8 and 12 bytes past a 256-byte boundary, byte masks at 1, 3, 8 and 15, bit words at 8: all of them up to 8257 frames,
offset 0 and one off-grid placement beyond.

The closing test asserts that the names recorded over the module cover every launch name that receives a caller's pointer."""
import os

import numpy as np
import pytest

import dispatch_ledger as L
import guarded as G
from fast_dnn_amd import api, convert as CV, formats as F

pytestmark = pytest.mark.gpu

SEEN = set()          # launch names recorded under guarded runs, over the module
SEEN_OTHER = set()    # the kernels with counters of their own (lists, union, top-k, float net, report)

# placements: byte offsets past a 256-byte boundary per buffer kind.  x: the quantized net's frames (multiples of 16);
# f: other float / int32 buffers; b: byte masks; w: bit words
PLACEMENTS = (dict(x=0, f=0, b=0, w=0), dict(x=16, f=4, b=1, w=8), dict(x=0, f=8, b=3, w=0), dict(x=48, f=12, b=8, w=8), dict(x=112, f=4, b=15, w=8))
LARGE = (PLACEMENTS[0], dict(x=16, f=12, b=3, w=8))
ACTIVE_BYTES = np.array([1, 2, 127, -128, -1], np.int8)


def placements(n):
    return PLACEMENTS if n <= 8257 else LARGE


@pytest.fixture(scope="module")
def torch():
    import torch as t

    yield t
    api.launch_record(False)
    for f in (api.set_fuse, api.set_chain, api.set_pp, api.set_ppo):
        f(-1)
    L.release_models()
    _X.clear()
    _M.clear()


# ------------------------------------------------------------------------------------------------------------- inputs
_X, _M = {}, {}


def features(n, D):
    if (n, D) not in _X:
        _X[(n, D)] = F.synth_features(n, D, seed=1000 + n % 977, pad_from=None if D != 432 else 429)
    return _X[(n, D)]


def masks01(n, O):
    """0 / 1 masks [n][O] at 40 % (the ledger's generators); one set per n, cut to the width."""
    W = -(-O // 256) * 256
    if (n, W) not in _M:
        gen = F.generate_masks_fast if n * W > (1 << 22) else F.generate_masks  # (same statistics; the per-frame loop costs seconds)
        _M[(n, W)] = gen(n, W, 0.40, 0.03, seed=7 + n % 89)
    return np.ascontiguousarray(_M[(n, W)][:, :O])


def dirty_bytes(m01, seed):
    """The same mask with every active byte drawn from {1, 2, 127, -128, -1}: 0x80 and 0x01 in every position of a 4-byte
    group and of a 16-byte piece (asserted where the mask is large enough to expect it)."""
    rng = np.random.default_rng(seed)
    d = np.where(m01 != 0, ACTIVE_BYTES[rng.integers(0, 5, m01.shape)], 0).astype(np.int8)
    if 16 * 400 <= m01.size <= 1 << 22:
        flat_pos = np.arange(m01.size).reshape(m01.shape) % 16
        for v in (-128, 1):
            assert set(np.unique(flat_pos[d == v])) == set(range(16)), v
    return d


def stray_bits(m01, seed):
    """The mask as bit words, as int64; for O % 64 != 0 with random bits past O in every row's last word."""
    n, O = m01.shape
    bits = F.pack_mask_bits(m01).copy()
    if O % 64:
        rng = np.random.default_rng(seed)
        junk = rng.integers(0, 1 << 63, n, dtype=np.uint64) << np.uint64(O % 64)
        bits[:, -1] |= junk
        assert (bits[:, -1] >> np.uint64(O % 64)).any()
    return bits.view(np.int64)


def sample(n, T, seed):
    pick = {0, n - 1} | {r for r in (T - 1, T) if 0 <= r < n}
    rng = np.random.default_rng(seed)
    while len(pick) < min(n, 36):
        pick.add(int(rng.integers(0, n)))
    return np.array(sorted(pick))


# ------------------------------------------------------------------------------------------------------------ buffers
class Spec:
    """One device buffer of a call.  kind 'x' | 'f' | 'b' | 'w' picks the placement's offset; data: an array (input) or an
    element count (output); width: the row length the guard sizes come from; fill: poison of an input."""

    def __init__(self, name, kind, dtype, data, width, fill=None, clean=None):
        self.name, self.kind, self.dtype, self.data, self.width, self.fill, self.clean = name, kind, dtype, data, width, fill, clean

    @property
    def is_input(self):
        return not isinstance(self.data, (int, np.integer))


def place(torch, specs, pl):
    """pl None: fresh, exactly sized buffers (inputs: the CLEAN form where a spec has one); else guarded at the placement."""
    out = {}
    for s in specs:
        dt = getattr(torch, s.dtype)
        if pl is None:
            if s.is_input:
                t = torch.from_numpy(np.ascontiguousarray(s.clean if s.clean is not None else s.data).reshape(-1)).cuda()
            else:
                t = torch.zeros(int(s.data), dtype=dt, device="cuda")
            assert t.data_ptr() % 256 == 0
            out[s.name] = t
        elif s.is_input:
            head, tail = G.in_guard(s.width)
            out[s.name] = G.guarded(s.data, dt, head, tail, pl[s.kind], fill=s.fill, device="cuda", name=s.name)
        else:
            out[s.name] = G.guarded(int(s.data), dt, G.out_guard(s.width), G.out_guard(s.width), pl[s.kind], device="cuda", name=s.name)
    return out


def ptrs(bufs):
    return {k: (v.ptr if isinstance(v, G.Guarded) else v.data_ptr()) for k, v in bufs.items()}


def payload(buf):
    return buf.view if isinstance(buf, G.Guarded) else buf


def same_bits(torch, a, b):
    bits = {1: torch.uint8, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.view(bits), b.view(bits))


def run_everywhere(torch, specs, call, n, what, must=()):
    """The call on plain buffers, then guarded at every placement for n: (a) and (b); -> (plain buffers, the guarded
    buffers of the first off-grid placement, for (c))."""
    plain = place(torch, specs, None)
    call(ptrs(plain))
    torch.cuda.synchronize()
    keep = None
    for i, pl in enumerate(placements(n)):
        bufs = place(torch, specs, pl)
        torch.cuda.synchronize()
        _, names = L.launched(lambda: (call(ptrs(bufs)), torch.cuda.synchronize()))
        SEEN.update(names)
        missing = set(must) - names
        if i == 0:  # (the instances that need a buffer ON the grid -- norm.small, maskpack.flat -- are asked for there only)
            assert not missing, f"{what}: {sorted(missing)} did not run; ran {sorted(names)}"
        else:
            assert not (missing - {"norm.small", "maskpack.flat"}), f"{what} @ {pl}: {sorted(missing)} did not run; ran {sorted(names)}"
        for s in specs:
            bufs[s.name].check(f"{what} @ {pl}")
            if not s.is_input:
                assert same_bits(torch, bufs[s.name].view, plain[s.name]), f"{what} @ {pl}: {s.name} differs from the plain buffers' bytes"
        if i == 1:
            keep = bufs
    return plain, keep


def rows_of(torch, buf, n, O, idx):
    return payload(buf).view(n, O)[torch.from_numpy(idx).cuda()].cpu().numpy()


def oracle_rows(case_id, orc, x, idx, masks, dense=None, lazy=(), soft=True):
    """(c): the ledger's checks on the sampled rows.  dense / lazy: [len(idx)][O] arrays."""
    if not soft:
        return
    hid = orc.hidden_acts_mt(x[idx])
    want, acc = orc.output_mt(hid, want_acc=True)
    if dense is not None:
        L._softmax_ok(dense, want, case_id + " dense")
        L._softmax_rel_ok(dense, want, orc, acc, case_id + " dense")
    if len(lazy):
        want_lazy = orc.output_mt(hid, masks=masks[idx])
        for tag, got in lazy:
            L._softmax_ok(got, want_lazy, f"{case_id} {tag}")
            L._softmax_rel_ok(got, want_lazy, orc, acc, f"{case_id} {tag}", masks=masks[idx])
            L._masked_out_ok(got, masks[idx], f"{case_id} {tag}")


class modes:
    def __init__(self, fuse=-1, chain=(-1, 0), pp=(-1, 0), ppo=-1):
        self.v = (fuse, chain, pp, ppo)

    def __enter__(self):
        fuse, chain, pp, ppo = self.v
        api.set_fuse(fuse), api.set_chain(*chain), api.set_pp(*pp), api.set_ppo(ppo)

    def __exit__(self, *a):
        api.set_fuse(-1), api.set_chain(-1), api.set_pp(-1), api.set_ppo(-1)


def model(net):
    return L._model(L.Case("caller_buffers", net, 0, "prod", ()))


# ------------------------------------------------------------------------- the output instances through a context's forms
def _out_names(shape, width, fuse, nofix=False):
    anyw = width % 32 != 0
    if shape == "small":
        return ("small.out.prod", "small.out.masked", "maskunpack")
    if fuse:
        tail = "_nofix" if nofix else "_anyw" if anyw else ""
        return (f"gemm.out.{shape}.fused{tail}", f"gemm.out.{shape}.fused_masked{tail}")
    return (f"gemm.out.{shape}." + ("anyw" if anyw else "plain"), f"gemm.out.{shape}." + ("masked_anyw" if anyw else "masked"))


CTX_CASES = []  # (id, net, n, tile, fuse, must)
for _w in (256, 251):
    CTX_CASES.append((f"small.w{_w}.n33", f"n256/{_w}/gauss", 33, 32, 0, _out_names("small", _w, 0) + (("norm.small",) if _w == 256 else ("norm.rows",))))
    for _n, _T, _shape in ((545, 32, "ft32"), (8257, 64, "ft64"), (16513, 128, "ft128.bk128"), (33025, 256, "ft256"), (65601, 320, "ft320")):
        CTX_CASES.append((f"{_shape}.unfused.w{_w}.n{_n}", f"n256/{_w}/gauss", _n, _T, 0,  # (norm.small: up to 1024 rows of whole 16-byte groups)
                          _out_names(_shape, _w, 0) + ("norm.small" if _n <= 1024 and _w == 256 else "norm.rows", "maskpack.flat" if _w == 256 else "maskpack.rows")))
        if _T >= 128:
            CTX_CASES.append((f"{_shape}.fused.w{_w}.n{_n}", f"n256/{_w}/gauss", _n, _T, 1, _out_names(_shape, _w, 1)))
    CTX_CASES.append((f"tdiv.w{_w}.n129", f"tdiv/{_w}", 129, 128, 0, _out_names("tdiv", _w, 0)))
for _n, _T in ((33025, 256), (65601, 320)):
    CTX_CASES.append((f"ft{_T}.fused_nofix.n{_n}", "n256/256/nosat", _n, _T, 1, _out_names(f"ft{_T}", 256, 1, nofix=True)))
# the 64-byte-step 128-frame shape: single-tile launches of a 129-node-tile layer (the ledger's wout cases; 321 .. 384 frames)
CTX_CASES.append(("wout.ft128.w33024.n321", "wout/33024", 321, 128, 0, ("gemm.out.ft128.plain", "gemm.out.ft128.masked")))
CTX_CASES.append(("wout.ft128.w33021.n383", "wout/33021", 383, 128, 0, ("gemm.out.ft128.anyw", "gemm.out.ft128.masked_anyw")))


@pytest.mark.parametrize("cid,net,n,T,fuse,must", CTX_CASES, ids=[c[0] for c in CTX_CASES])
def test_context_forms_on_guarded_buffers(torch, cid, net, n, T, fuse, must):
    """fdnn_ctx_forward_hidden_device, fdnn_ctx_output_device, fdnn_ctx_lazy_output_batch_device and
    fdnn_ctx_lazy_output_batch_bits_device (whole range, and a sub-range first > 0 that takes the small-batch kernels behind
    maskunpack), all buffers of the four calls guarded at once.  The plain run has clean masks, the guarded runs dirty bytes
    and stray bits."""
    path, dnn, orc = model(net)
    D, O = dnn.inputDimension(), dnn.outputDimension()
    x, m01 = features(n, D), masks01(n, O)
    first = n - 32 if n > 33 else 1
    sub = n - first
    specs = [Spec("x", "x", "float32", x, D, fill=float("nan")),
             Spec("masks", "b", "int8", dirty_bytes(m01, n), O, fill=-128, clean=m01.astype(np.int8)),
             Spec("bits", "w", "int64", stray_bits(m01, n), (O + 63) // 64, fill=-1, clean=F.pack_mask_bits(m01).view(np.int64)),
             Spec("dense", "f", "float32", n * O, O), Spec("lazy", "f", "float32", n * O, O), Spec("lazyb", "f", "float32", n * O, O),
             Spec("sub", "f", "float32", sub * O, O)]
    wpr = (O + 63) // 64
    ctx = dnn.getNewLazyContext(n)

    def call(p):
        ctx.calculateUntilOutputDevice(p["x"])
        lib = api.lib()
        api._check(lib.fdnn_ctx_output_device(ctx.handle, p["dense"], None))
        ctx.calculateForOutputNodesBatchDevice(p["masks"], p["lazy"], 0, n)
        ctx.calculateForOutputNodesBatchBitsDevice(p["bits"], p["lazyb"], 0, n)
        ctx.calculateForOutputNodesBatchBitsDevice(p["bits"] + 8 * wpr * first, p["sub"], first, sub)

    try:
        with modes(fuse=fuse, chain=(0, 0)):
            plain, kept = run_everywhere(torch, specs, call, n, cid, must=must)
    finally:
        ctx.delete()
    assert same_bits(torch, plain["lazy"], plain["lazyb"]), f"{cid}: byte masks and bit masks give other bytes"
    assert same_bits(torch, plain["sub"], plain["lazyb"][first * O:]), f"{cid}: a sub-range's rows differ from the whole range's"
    idx = sample(n, T, seed=n)
    oracle_rows(cid, orc, x, idx, m01, dense=rows_of(torch, kept["dense"], n, O, idx),
                lazy=(("lazy bytes", rows_of(torch, kept["lazy"], n, O, idx)), ("lazy bits", rows_of(torch, kept["lazyb"], n, O, idx))),
                soft=not net.startswith("tdiv"))  # (the ledger holds the infinite-multiplier nets to integer state only: no soft-max bar exists for them)


# ---------------------------------------------------------------------------------------- the pooled dense / bit-mask calls
POOLED = [("n256/251/gauss", 545, 32, -1, ("gemm.out.ft32.anyw", "gemm.out.ft32.masked_anyw", "norm.rows")),
          ("n256/251/gauss", 20480 + 545, 32, -1, ("gemm.out.ft32.anyw", "gemm.out.ft32.masked_anyw")),  # two chunks: 20480 + 545 rows
          ("full/gauss", 641, 320, 1, ("ppo.out.fix",)), ("full/nosat", 641, 320, 1, ("ppo.out.nofix",))]


@pytest.mark.parametrize("net,n,T,ppo,must", POOLED, ids=[f"{c[0]}.n{c[1]}" for c in POOLED])
def test_pooled_calls_on_guarded_buffers(torch, net, n, T, ppo, must):
    """fdnn_calculate_device and fdnn_calculate_lazy_bits_device; one call long enough to go as two chunks with O = 251 (the
    second chunk's d_out + off * O keeps the base's offset: chunk starts are multiples of 10240 rows), and the role-split
    fused output kernel forced on the full net (641 frames: the third 320-frame tile has one live row)."""
    path, dnn, orc = model(net)
    D, O = dnn.inputDimension(), dnn.outputDimension()
    if n > 20480:
        assert len(api.frame_chunks(n, True)) == 2 and len(api.frame_chunks(n, False)) == 2
    x, m01 = features(n, D), masks01(n, O)
    specs = [Spec("x", "x", "float32", x, D, fill=float("nan")),
             Spec("bits", "w", "int64", stray_bits(m01, n), (O + 63) // 64, fill=-1, clean=F.pack_mask_bits(m01).view(np.int64)),
             Spec("dense", "f", "float32", n * O, O), Spec("lazy", "f", "float32", n * O, O)]

    def call(p):
        dnn.calculate_device(p["x"], n, p["dense"])
        dnn.calculate_lazy_bits_device(p["x"], n, p["bits"], p["lazy"])

    with modes(fuse=1 if ppo == 1 else -1, ppo=ppo):
        plain, kept = run_everywhere(torch, specs, call, n, f"pooled {net} n {n}", must=must)
    idx = np.unique(np.concatenate((sample(n, T, seed=n), [20479, 20480] if n > 20480 else [])).astype(np.int64))
    oracle_rows(f"pooled {net} n {n}", orc, x, idx, m01, dense=rows_of(torch, kept["dense"], n, O, idx),
                lazy=(("lazy bits", rows_of(torch, kept["lazy"], n, O, idx)),))


# ------------------------------------------------------------------------------------ layer 0: every kernel that reads d_x
L0_CASES = [(100, 0, False, ("l0.small.prod",)), (300, 2, False, ("l0.tile16.prod",)), (1000, 2, False, ("l0.tile32.prod",)),
            (1201, 2, False, ("l0.tile64.prod",)), (700, 1, False, ("l0.image.frames",)), (600, 0, False, ("l0.digits", "l0.fixlist.lpo8")),
            (6177, 0, False, ("l0.digits", "l0.fixlist.lpo4")), (2048, 3, False, ("l0.screen.f128", "l0.fix.tiles")), (300, 0, True, ("l0.mfma.prod",))]


@pytest.mark.parametrize("n,kernel,fma,must", L0_CASES, ids=[f"{c[3][-1]}.n{c[0]}" for c in L0_CASES])
def test_layer0_reads_only_the_callers_rows(torch, n, kernel, fma, must):
    """fdnn_ctx_forward_hidden_device with each layer-0 kernel: NaN in front of and behind the frames must not reach the last
    hidden layer's bytes, which are the oracle's for every row."""
    from oracle.oracle import Oracle

    path, dnn, orc = model("mid")
    D = dnn.inputDimension()
    x = features(n, D)
    specs = [Spec("x", "x", "float32", x, D, fill=float("nan"))]
    ctx = dnn.getNewLazyContext(n)
    got = []
    dnn.setInputLayerKernel(kernel), dnn.setInputLayerFma(fma), Oracle.set_l0_fma(fma)
    try:
        def call(p):
            ctx.calculateUntilOutputDevice(p["x"])
            torch.cuda.synchronize()
            got.append(ctx.hiddenActivations())

        run_everywhere(torch, specs, call, n, f"l0 n {n} kernel {kernel}", must=must)
        want = orc.hidden_acts_mt(x)
    finally:
        dnn.setInputLayerKernel(0), dnn.setInputLayerFma(False), Oracle.set_l0_fma(False)
        ctx.delete()
    for i, h in enumerate(got):
        assert np.array_equal(h, want), f"l0 n {n} kernel {kernel}: run {i}: hidden bytes differ from the oracle"


# -------------------------------------------------------------------------------------------------- raw frames, spliced
def test_raw_frames_with_a_segment_table(torch):
    """fdnn_calculate_raw_device: d_raw [n][39] between NaN (a clamp that fails reads it), three utterances."""
    path, dnn, orc = model("mid")
    n, O, raw_dim, offsets = 300, dnn.outputDimension(), 39, list(range(-5, 6))
    raw = np.ascontiguousarray(features(n, 432)[:, :raw_dim])
    segs = [0, 100, 101]
    specs = [Spec("raw", "f", "float32", raw, raw_dim, fill=float("nan")), Spec("out", "f", "float32", n * O, O)]
    dnn.setSplice(offsets, raw_dim)
    try:
        plain, kept = run_everywhere(torch, specs, lambda p: dnn.calculateRawDevice(p["raw"], n, p["out"], segStarts=segs), n, "raw", must=("splice",))
    finally:
        dnn.setSplice([], 0)
    x = np.concatenate([CV.splice_frames(raw[a:b], offsets, 432) for a, b in zip(segs, segs[1:] + [n])])
    idx = np.arange(n)
    oracle_rows("raw", orc, x, idx, None, dense=rows_of(torch, kept["out"], n, O, idx))


# ------------------------------------------------------------------------------------------------------ the scoring loop
@pytest.mark.parametrize("masked", [False, True], ids=["dense", "masks"])
def test_server_submit_device(torch, masked):
    path, dnn, orc = model("mid")
    n, D, O = 300, dnn.inputDimension(), dnn.outputDimension()
    x, m01 = features(n, D), masks01(n, O)
    specs = [Spec("x", "x", "float32", x, D, fill=float("nan")), Spec("out", "f", "float32", n * O, O)]
    if masked:
        specs.append(Spec("masks", "b", "int8", dirty_bytes(m01, 5), O, fill=1, clean=m01.astype(np.int8)))
    srv = api.ScoringServer(dnn, 512, 2)
    try:
        def call(p):
            srv.wait(srv.submit_device(p["x"], n, p["out"], p.get("masks", 0)))

        with modes(fuse=0):
            plain, kept = run_everywhere(torch, specs, call, n, f"server masked={masked}", must=("small.out.masked",) if masked else ("small.out.prod", "norm.small"))
    finally:
        srv.close()
    idx = np.arange(n)
    got = rows_of(torch, kept["out"], n, O, idx)
    oracle_rows("server", orc, x, idx, m01, dense=None if masked else got, lazy=(("lazy", got),) if masked else ())


# ---------------------------------------------------------------------------------------------------------------- lists
@pytest.mark.parametrize("union", [0, 2], ids=["dot", "union"])
def test_lists_device_form(torch, union):
    """fdnn_ctx_lazy_output_lists_device: row_ptr / nodes between negative indices, probs [nnz] and inactive [count] guarded;
    rows first > 0 of the context."""
    path, dnn, orc = model("mid")
    n, first, D, O = 300, 7, dnn.inputDimension(), dnn.outputDimension()
    count = n - first
    x, m01 = features(n, D), masks01(n, O)
    rp, nd = F.masks_to_lists(m01[first:])
    nnz = int(rp[-1])
    specs = [Spec("rp", "f", "int32", rp, count + 1, fill=G.INT_SENTINEL), Spec("nd", "f", "int32", nd, O, fill=G.INT_SENTINEL),
             Spec("probs", "f", "float32", nnz, O), Spec("inactive", "f", "float32", count, O)]
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutput(x)
    dnn.setListsUnion(union)
    try:
        before = api.lists_launches(), api.lists_union_launches()
        plain, kept = run_everywhere(torch, specs, lambda p: ctx.calculateForOutputNodesListsDevice(p["rp"], p["nd"], nnz, p["probs"], p["inactive"], first, count),
                                     n, f"lists union={union}")
        after = api.lists_launches(), api.lists_union_launches()
    finally:
        dnn.setListsUnion(0)
        ctx.delete()
    assert after[0][2] > before[0][2], "the finish kernel did not run"
    if union:
        assert after[1][0] > before[1][0] and sum(after[1][1:3]) > sum(before[1][1:3]) and after[1][3] == before[1][3], "the union path did not serve the call"
        SEEN_OTHER.update(("lists.union.build", "lists.union.score", "lists.finish"))
    else:
        assert sum(after[0][:2]) > sum(before[0][:2]), "the dot-product score kernel did not run"
        SEEN_OTHER.update(("lists.score", "lists.finish"))
    rows = F.lists_to_rows(rp, nd, payload(kept["probs"]).cpu().numpy(), payload(kept["inactive"]).cpu().numpy(), O)
    idx = np.arange(count)
    oracle_rows(f"lists union={union}", orc, x[first:], idx, m01[first:], lazy=(("lists", rows),))


def test_set_and_sets_device_forms(torch):
    """fdnn_ctx_lazy_output_set_device and fdnn_ctx_lazy_output_sets_device off the grid (their own tests plant sentinels behind
    exactly placed buffers): the rows they stand for are the oracle's lazy rows under the sets' masks."""
    path, dnn, orc = model("mid")
    n, D, O = 300, dnn.inputDimension(), dnn.outputDimension()
    x, m01 = features(n, D), masks01(n, O)
    s0, s1 = np.flatnonzero(m01[5]).astype(np.int32), np.flatnonzero(m01[200]).astype(np.int32)[:77]
    seg_rows, set_ptr = [0, 33, n], [0, s0.size, s0.size + s1.size]
    nnz = 33 * s0.size + (n - 33) * s1.size
    specs = [Spec("set", "f", "int32", s0, O, fill=G.INT_SENTINEL), Spec("sets", "f", "int32", np.concatenate((s0, s1)), O, fill=G.INT_SENTINEL),
             Spec("p1", "f", "float32", (n - 7) * s0.size, s0.size), Spec("i1", "f", "float32", n - 7, O),
             Spec("p2", "f", "float32", nnz, O), Spec("i2", "f", "float32", n, O)]
    ctx = dnn.getNewLazyContext(n)
    ctx.calculateUntilOutput(x)

    def call(p):
        ctx.calculateForOutputNodeSetDevice(p["set"], s0.size, p["p1"], p["i1"], 7, n - 7)
        ctx.calculateForOutputNodeSetsDevice(seg_rows, set_ptr, p["sets"], p["p2"], p["i2"])

    before = api.set_launches(), api.sets_launches()
    try:
        plain, kept = run_everywhere(torch, specs, call, n, "set / sets")
    finally:
        ctx.delete()
    after = api.set_launches(), api.sets_launches()
    assert sum(after[0]) > sum(before[0]) and sum(after[1]) > sum(before[1])
    p1, i1 = payload(kept["p1"]).view(n - 7, s0.size).cpu().numpy(), payload(kept["i1"]).cpu().numpy()
    p2, i2 = payload(kept["p2"]).cpu().numpy(), payload(kept["i2"]).cpu().numpy()
    mask0, mask1 = np.zeros(O, np.int8), np.zeros(O, np.int8)
    mask0[s0], mask1[s1] = 1, 1
    rows1 = np.repeat(i1[:, None], O, axis=1)
    rows1[:, s0] = p1
    oracle_rows("set", orc, x[7:], np.arange(n - 7), np.tile(mask0, (n - 7, 1)), lazy=(("set", rows1),))
    rows2 = np.repeat(i2[:, None], O, axis=1)
    rows2[:33, s0] = p2[:33 * s0.size].reshape(33, s0.size)
    rows2[33:, s1] = p2[33 * s0.size:].reshape(n - 33, s1.size)
    oracle_rows("sets", orc, x, np.arange(n), np.concatenate((np.tile(mask0, (33, 1)), np.tile(mask1, (n - 33, 1)))), lazy=(("sets", rows2),))


def test_topk_rows_device_outputs_off_the_grid(torch):
    """fdnn_topk_rows_device with all three buffers guarded (tests/test_gpu_topk_rows.py moves the rows alone): the contract
    stated in numpy (tests/topk_cases.py) on the same rows."""
    import topk_cases as TC

    n, width, k = 37, 1001, 65
    rows = TC.rows_of("softmax", n, width, k, seed=2)
    specs = [Spec("rows", "f", "float32", rows, width, fill=float("nan")), Spec("nodes", "f", "int32", n * k, k), Spec("vals", "f", "float32", n * k, k)]
    plain, kept = run_everywhere(torch, specs, lambda p: api.topk_rows_device(p["rows"], n, width, k, p["nodes"], p["vals"]), n, "topk rows")
    want = TC.select(rows, k)
    assert np.array_equal(payload(kept["nodes"]).view(n, k).cpu().numpy(), want[0])
    assert np.array_equal(payload(kept["vals"]).view(n, k).cpu().numpy().view(np.uint32), want[1])


# ---------------------------------------------------------------------------------------------------------------- top-k
@pytest.mark.parametrize("form", ["ctx", "model"])
def test_topk_device_forms(torch, form):
    """fdnn_ctx_output_topk_device / fdnn_calculate_topk_device: nodes int32 [n][k] and probs [n][k] guarded.  Against the
    oracle: every returned probability within the soft-max bar of the oracle's at that node, and no node left out whose
    oracle probability exceeds the smallest returned one by more than twice the bar."""
    path, dnn, orc = model("mid")
    n, k, D, O = 300, 5, dnn.inputDimension(), dnn.outputDimension()
    x = features(n, D)
    specs = [Spec("nodes", "f", "int32", n * k, k), Spec("probs", "f", "float32", n * k, k)]
    ctx = None
    if form == "ctx":
        ctx = dnn.getNewLazyContext(n)
        ctx.calculateUntilOutput(x)
        call = lambda p: ctx.calculateOutputTopKDevice(k, p["nodes"], p["probs"])  # noqa: E731
    else:
        specs.insert(0, Spec("x", "x", "float32", x, D, fill=float("nan")))
        call = lambda p: dnn.calculate_topk_device(p["x"], n, k, p["nodes"], p["probs"])  # noqa: E731
    before = api.topk_launches()
    try:
        plain, kept = run_everywhere(torch, specs, call, n, f"topk {form}")
    finally:
        if ctx is not None:
            ctx.delete()
    assert sum(api.topk_launches()) > sum(before)
    SEEN_OTHER.add("topk")
    nodes, probs = payload(kept["nodes"]).view(n, k).cpu().numpy(), payload(kept["probs"]).view(n, k).cpu().numpy()
    want = orc.calculate(x)
    assert (nodes >= 0).all() and (nodes < O).all() and all(len(set(r)) == k for r in nodes)
    at = np.take_along_axis(want, nodes, axis=1)
    assert np.abs(probs - at).max() <= L.TIGHT
    rest = want.copy()
    np.put_along_axis(rest, nodes, -np.inf, axis=1)
    assert (rest.max(1) <= at.min(1) + 2 * L.TIGHT).all() and (np.diff(probs, axis=1) <= 0).all()


# ------------------------------------------------------------------------------------------- the float net and the report
def test_float_net_and_report(torch, tmp_models):
    """fdnn_float_calculate_device (its input step reads d_x by scalar loads: element alignment) and fdnn_report_add_device
    (inputs only).  Reference: the net in float64 numpy; sums of at most 48 fp32 products leave the logits within ~1e-5 and a
    probability (< 1) within the suite's 2e-6."""
    net = F.synth_net([20, 48, 48, 48, 131], seed=21, w0_std=0.05, w_std=0.3)
    p = os.path.join(tmp_models, "caller_buffers_float.bin")
    F.write_model_bin(p, net)
    dnn = api.FloatDnn.loadFromFile(p, device=0)
    n, D, O = 300, 20, 131
    x = F.synth_features(n, D, seed=4, pad_from=None)
    specs = [Spec("x", "f", "float32", x, D, fill=float("nan")), Spec("out", "f", "float32", n * O, O)]
    before = api.float_launches()
    try:
        plain, kept = run_everywhere(torch, specs, lambda q: dnn.calculateDevice(q["x"], n, q["out"]), n, "float net")
    finally:
        dnn.delete()
    after = api.float_launches()
    assert after["input_step"] > before["input_step"] and after["fgemm.exp"] > before["fgemm.exp"]
    SEEN_OTHER.add("float.input_step")
    got = payload(kept["out"]).view(n, O).cpu().numpy()
    a = (x.astype(np.float64) + net.shift.astype(np.float64)) * net.scale.astype(np.float64)
    for j, l in enumerate(net.layers):
        z = a @ l.weights.astype(np.float64).T + l.bias.astype(np.float64)
        a = 1.0 / (1.0 + np.exp(-z)) if j + 1 < len(net.layers) else None
    e = np.exp(z - z.max(1, keepdims=True))
    want = e / e.sum(1, keepdims=True)
    assert np.abs(got - want).max() <= L.TIGHT

    q = (got + np.float32(1e-3) * np.random.default_rng(1).standard_normal(got.shape).astype(np.float32)).astype(np.float32)
    q[17, 5] = np.nan
    rspecs = [Spec("ref", "f", "float32", got, O, fill=float("nan")), Spec("q", "f", "float32", q, O, fill=float("nan"))]
    rep = api.AccuracyReport(O, device=0)
    try:
        for pl in PLACEMENTS:
            bufs = place(torch, rspecs, pl)
            rep.reset()
            rep.addDevice(bufs["ref"].ptr, bufs["q"].ptr, n)
            acc = rep.read(0.1)
            torch.cuda.synchronize()
            bufs["ref"].check("report"), bufs["q"].check("report")
            ok = np.arange(n) != 17
            d = np.abs(q[ok].astype(np.float64) - got[ok].astype(np.float64))
            assert acc["frames"] == n and acc["nan_rows"] == 1 and acc["max_abs_diff"] == float(d.max()), (pl, acc)
            assert acc["top1_agree_rows"] == int((q[ok].argmax(1) == got[ok].argmax(1)).sum()), pl
            assert abs(acc["sum_abs_diff"] - float(d.sum())) <= 1e-9 * float(d.sum()), pl
    finally:
        rep.delete()
    assert api.float_launches()["report.rows"] > after["report.rows"]
    SEEN_OTHER.add("report")


# --------------------------------------------------------------------------------- the one requirement wider than an element
def test_frames_off_16_bytes_are_refused_before_any_launch(torch):
    """d_x of the quantized net is the source of layer 0's 16-byte LDS-DMA: frames that do not start on a 16-byte boundary are
    FDNN_E_ARG from every entry point that takes them, nothing is launched and no output is touched."""
    path, dnn, orc = model("mid")
    n, k, D, O = 100, 5, dnn.inputDimension(), dnn.outputDimension()
    x, m01 = features(n, D), masks01(n, O)
    ctx = dnn.getNewLazyContext(n)
    srv = api.ScoringServer(dnn, 512, 2)
    try:
        for off in (4, 8, 12):
            specs = [Spec("x", "f", "float32", x, D, fill=float("nan")), Spec("bits", "w", "int64", F.pack_mask_bits(m01).view(np.int64), (O + 63) // 64, fill=-1),
                     Spec("out", "f", "float32", n * O, O), Spec("nodes", "f", "int32", n * k, k), Spec("probs", "f", "float32", n * k, k)]
            b = place(torch, specs, dict(f=off, w=8))
            p = ptrs(b)
            assert p["x"] % 16 == off
            torch.cuda.synchronize()
            other = api.topk_launches(), api.lists_launches()
            api.launch_record(True)
            api.launch_reset()
            try:
                for call in (lambda: dnn.calculate_device(p["x"], n, p["out"]), lambda: dnn.calculate_lazy_bits_device(p["x"], n, p["bits"], p["out"]),
                             lambda: ctx.calculateUntilOutputDevice(p["x"]), lambda: dnn.calculate_topk_device(p["x"], n, k, p["nodes"], p["probs"]),
                             lambda: srv.submit_device(p["x"], n, p["out"])):
                    with pytest.raises(api.FdnnError) as e:
                        call()
                    assert e.value.code == api.FDNN_E_ARG and "16-byte" in str(e.value)
                torch.cuda.synchronize()
                assert api.launch_counts() == {}, "a refused call launched something"
            finally:
                api.launch_record(False)
            assert (api.topk_launches(), api.lists_launches()) == other
            for g in b.values():
                g.assert_untouched(f"frames at +{off}")
            with pytest.raises(api.FdnnError) as e:  # (the context is as it was: no hidden layers yet)
                api._check(api.lib().fdnn_ctx_output_device(ctx.handle, p["out"], None))
            assert e.value.code == api.FDNN_E_STATE
    finally:
        srv.close()
        ctx.delete()


# ------------------------------------------------------------------ stray mask bits and byte values through the host forms
@pytest.mark.parametrize("net,n", [("mid", 300), ("n256/251/gauss", 8257)])
def test_dirty_masks_through_the_host_forms(torch, net, n):
    """"non-zero = active" and "bits past output_dim ignored" where the result comes back compacted and is expanded on the
    host: fdnn_calculate_lazy, fdnn_calculate_lazy_bits, fdnn_ctx_lazy_output_batch_bits and submitLazy return the clean masks' bytes."""
    path, dnn, orc = model(net)
    D, O = dnn.inputDimension(), dnn.outputDimension()
    x, m01 = features(n, D), masks01(n, O)
    clean_bits, stray = F.pack_mask_bits(m01), stray_bits(m01, n).view(np.uint64)
    want = dnn.calculateLazy(x, masks=m01.astype(np.int8)).view(np.uint32)
    assert np.array_equal(dnn.calculateLazy(x, masks=dirty_bytes(m01, n)).view(np.uint32), want)
    assert np.array_equal(dnn.calculateLazy(x, bits=clean_bits).view(np.uint32), want)
    assert np.array_equal(dnn.calculateLazy(x, bits=stray).view(np.uint32), want)
    ctx = dnn.getNewLazyContext(n)
    try:
        ctx.calculateUntilOutput(x)
        assert np.array_equal(ctx.calculateForOutputNodesBatchBits(stray).view(np.uint32), want)
        assert np.array_equal(ctx.calculateForOutputNodesBatch(dirty_bytes(m01, n + 1)).view(np.uint32), want)
    finally:
        ctx.delete()
    srv = api.ScoringServer(dnn, 16384, 2)
    try:
        t, out = srv.submitLazy(x, stray)
        srv.wait(t)
        assert np.array_equal(out.view(np.uint32), want)
    finally:
        srv.close()
    idx = sample(n, 64, seed=n)
    oracle_rows(f"host forms {net}", orc, x, idx, m01, lazy=(("lazy", want.view(np.float32)[idx]),))


# ------------------------------------------------------------------------------------------------------ the coverage gate
# Launch names whose kernel receives a caller's pointer: by prefix from the library's table, minus the names below.
CALLER_PREFIXES = ("small.out.", "gemm.out.", "ppo.out.", "norm.", "maskpack.", "maskunpack", "l0.", "splice")
_TAP = "a tap instance: only fdnn_debug_forward_taps launches it, on the context's own frame, mask and result buffers (fdnn_debug.cpp)"
_IMAGE = "reads p.xt, the transposed frame image l0.image.frames wrote into context scratch (fdnn_l0.hip: issue(), uniform_rsrc(p.xt ...)); never p.x"
_DIGITS = "reads p.xd, the digit planes l0.digits wrote into context scratch (fdnn_l0s.hip: rsrc_x over p.xd); never p.x"
NO_CALLER_POINTER = {
    "l0.split.n64": _DIGITS, "l0.split.n128": _DIGITS,
    "l0.split.n128.probe": "fdnn_debug_layer0_screen only, on frames the call uploads into context scratch (fdnn_debug.cpp); reads p.xd like l0.split.n128",
    **{f"l0.chain.jc{j}.tn{t}.prod": _IMAGE for j in (12, 16) for t in (64, 128)},
}
NO_CALLER_POINTER_BY_SUFFIX = {".tap": _TAP}
OTHER_REQUIRED = {"lists.score", "lists.finish", "lists.union.build", "lists.union.score", "topk", "float.input_step", "report"}


def required_names():
    out = set()
    for name, flags in api.launch_names().items():
        if flags or not name.startswith(CALLER_PREFIXES):  # (ablation-only and load-time names: no caller buffer exists then)
            continue
        if name not in NO_CALLER_POINTER and not name.endswith(tuple(NO_CALLER_POINTER_BY_SUFFIX)):
            out.add(name)
    return out


def test_every_instance_that_takes_a_callers_pointer_ran_guarded():
    assert all(k in api.launch_names() for k in NO_CALLER_POINTER), "an exclusion names no launch"
    missing = required_names() - SEEN
    assert not missing, f"no guarded case launched {sorted(missing)}"
    assert OTHER_REQUIRED <= SEEN_OTHER, sorted(OTHER_REQUIRED - SEEN_OTHER)
