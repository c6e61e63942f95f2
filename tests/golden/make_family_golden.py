#!/usr/bin/env python3
"""Record every family of tests/ref_families.py from the REFERENCE ITSELF -> tests/golden/families/*.npz, and the wider
quantizer cases -> tests/golden/quantizer_wide.npz.

Runs only where oracle/_ref/ has been built (oracle/Makefile: the reference's sources compiled where they lie, the plain
build -ffp-contract=off and the FMA build).  It drives oracle.RefLib / RefModel on synthetic features and stores DATA ONLY:
arrays and hashes.  It asserts every family's property (ref_families.properties) on the reference's recorded data alone and
asserts nothing on the oracle or the library; tests/test_oracle_families.py repeats those assertions from the fixtures.

    python tests/golden/make_family_golden.py [family ...]

The files are written with fixed zip time stamps: two runs give the same bytes.  No fixture may exceed 464 KB
(ref_families.MAX_FIXTURE_BYTES); families too large for that keep hashes of their integer state and a seeded sample of
columns of their float state (Family.sample).

Per family: the sha256 of the regenerated .bin and of the input rows, multipliers and hashes of the int8 weights, l0_lin,
every u8 layer, the float accumulator taps, logits, probabilities, the masks and lazy rows of a lazy family, the plain
build's l0_lin of an FMA family, the input rows of a hostile family, and the count of (frame, node) per int8 layer whose
accumulator is not the unsaturated dot product of the recorded bytes and weights."""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_families as RF  # noqa: E402
from fast_dnn_amd import formats as F  # noqa: E402
from oracle.oracle import RefLib  # noqa: E402

TMP = os.environ.get("TMPDIR", "/tmp")


def save(path, arrays):
    """np.savez_compressed with a fixed time stamp in every zip entry: the same arrays give the same bytes."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    size = os.path.getsize(path)
    assert size <= RF.MAX_FIXTURE_BYTES, f"{path}: {size} bytes > {RF.MAX_FIXTURE_BYTES}"
    return size


def same_taps(a, b):
    return all(np.array_equal(RF._bits(a[k]), RF._bits(b[k])) for k in a if k != "wq_sha256") and (a["wq_sha256"] == b["wq_sha256"]).all()


def family(fam, refs, done):
    path = RF.model(fam, TMP)
    ref = refs[fam.fma]
    probe = ref.load(path, fam.cutoff)
    in_dim, out_dim = probe.in_dim, probe.out_dim
    probe.close()
    x = RF.features(fam, in_dim)
    m = RF.masks(fam, out_dim) if fam.lazy else None
    taps = [RF.reference_taps(ref, fam, path, x, b, m) for b in fam.blocks]
    for b, t in zip(fam.blocks[1:], taps[1:]):
        assert same_taps(taps[0], t), f"{fam.name}: the reference's results at block size {b} differ from those at {fam.blocks[0]}"
    t = taps[0]
    g = RF.record(fam, t, F.sha256_file(path), x, m)
    wq = None
    if "events" in fam.props:
        wq = RF.int8_weights(path, fam, ref.quantize)
        assert [RF.sha(w) for w in wq] == list(t["wq_sha256"]), f"{fam.name}: the free-standing quantizer differs from the model's"
        g["events"] = np.array(RF.planted_events(t, wq), np.int64)
    if fam.fma:
        g["plain_l0_lin"] = RF.reference_taps(refs[False], fam, path, x, fam.blocks[0])["l0_lin"]
    figures = RF.properties(fam, g, wq=wq, plain_l0=g.get("plain_l0_lin"), base=done.get("plain"))
    size = save(os.path.join(HERE, fam.fixture), g)
    done[fam.name] = g
    return size, figures


def quantizer_cases():
    """(name, weights, cut-off) of quantizer_wide.npz.  Cut-offs <= 0 are rejected by the API (QuantizedDnn.java:55-57) and stay out."""
    rng = np.random.Generator(np.random.PCG64(199))
    gauss = (rng.standard_normal((32, 64)) * 1.5).astype(np.float32)
    cases = [(f"cut_{c}", gauss, c) for c in (0.5, 1.0, 2.0, 3.0, 4.0, float("inf"))]
    # ties: the dominant weight 127 / 64 fixes the multiplier at 64; (k + 0.5) / 64 is exact in fp32 and its product is k + 0.5
    ties = np.zeros((16, 16), np.float32)
    k = np.arange(-127, 127, dtype=np.float32)[:254]
    ties.ravel()[1:255] = (k + np.float32(0.5)) / np.float32(64.0)
    ties[0, 0] = np.float32(127.0 / 64.0)
    cases.append(("ties", ties, 3.0))
    for name, v in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf), ("3e38", 3e38), ("1e-41", 1e-41), ("negzero", -0.0)):
        w = (rng.standard_normal((16, 32)) * 0.3).astype(np.float32)
        w[5, 7] = np.float32(v)
        cases.append((f"plant_{name}", w, 3.0))
    cases.append(("all_denormal", (rng.standard_normal((16, 32)) * 1e-41).astype(np.float32), 3.0))
    cases.append(("const_0.25", np.full((16, 32), 0.25, np.float32), 3.0))
    cases.append(("m16x20", (rng.standard_normal((16, 20)) * 0.3).astype(np.float32), 3.0))
    return cases


def quantizer(ref):
    q = {}
    cases = quantizer_cases()
    with np.errstate(all="ignore"):
        for name, w, cut in cases:
            wq, mult = ref.quantize(w, cut)
            q[f"{name}_w"], q[f"{name}_cut"], q[f"{name}_wq"], q[f"{name}_mult"] = w, np.float32(cut), wq, np.float32(mult)
    q["names"] = np.array([c[0] for c in cases])
    # not blind: the cut-offs give different multipliers, and the ties round both ways from zero
    mults = [float(q[f"cut_{c}_mult"]) for c in (0.5, 1.0, 2.0, 3.0, 4.0, float("inf"))]
    assert len(set(mults)) == len(mults), mults
    assert float(q["ties_mult"]) == 64.0 and len(np.unique(q["ties_wq"])) > 200
    return save(os.path.join(HERE, "quantizer_wide.npz"), q), {"cut_mults": mults}


def main(argv):
    refs = {False: RefLib(), True: RefLib(fma=True)}
    names = argv or list(RF.NAMES)
    done, report = {}, {}
    if argv and any("cutoff" in RF.FAMILIES[n].props for n in names) and "plain" not in names:
        names = ["plain"] + names
    for n in names:
        size, figures = family(RF.FAMILIES[n], refs, done)
        report[n] = figures
        print(f"  {RF.FAMILIES[n].fixture:40s} {size:8d} B  {json.dumps(figures)}", flush=True)
    if not argv:
        size, figures = quantizer(refs[False])
        print(f"  {'quantizer_wide.npz':40s} {size:8d} B  {json.dumps(figures)}")


if __name__ == "__main__":
    main(sys.argv[1:])
