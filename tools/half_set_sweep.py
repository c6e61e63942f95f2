"""The half net's lazy output for node sets (fdnn_half_set.hip), measured on the bench net by the method of
tools/half_sweep.py: alternated in one process, warm-up, then ROUNDS blocks each; the median block, the spread (max - min) /
median.  Per frame count, for ONE 80-node set ("shared") and for per-utterance sets of 80 nodes over 100-frame segments
("utterances"):
  forward  fdnn_half_calculate_lazy_sets_device beside fdnn_half_calculate_device on the same frames -- the dense call is the
           only other way to the same numbers
  output   the set step alone (fdnn_debug_half_set_layer_us: row pointer, score, finish) beside the dense output layer alone
           (fdnn_debug_half_layer_us: exp launch, scale pass) on the same last hidden rows
The condition: the set form no slower than the dense one at every size, the margin the larger of the two spreads.  Before
anything is timed, the forward's set probabilities must have the bytes of the debug layer call on the same rows.

  python tools/half_set_sweep.py [--batches 100,1000,10000] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fast_dnn_amd import api  # noqa: E402
from fast_dnn_amd import formats as F  # noqa: E402
from half_sweep import ROUNDS, model_path, stats, timed  # noqa: E402

SET_LEN, SEG_FRAMES = 80, 100


def tables(kind, n, O, rng):
    """-> (seg_rows, set_ptr, nodes) covering [0, n)."""
    rows = [0, n] if kind == "shared" else list(range(0, n, SEG_FRAMES)) + [n]
    sets = [np.sort(rng.choice(O, SET_LEN, replace=False)).astype(np.int32) for _ in rows[1:]]
    return np.asarray(rows, np.int32), np.arange(len(rows), dtype=np.int32) * SET_LEN, np.concatenate(sets)


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="100,1000,10000")
    ap.add_argument("--out")
    args = ap.parse_args()
    hdnn = api.HalfDnn.loadFromFile(model_path())
    D, O, L = hdnn.inputDimension(), hdnn.outputDimension(), hdnn.layerCount()
    s = torch.cuda.current_stream().cuda_stream
    results, ok = [], True
    for n in (int(b) for b in args.batches.split(",")):
        x = F.synth_features(n, D, seed=500 + n)
        h = x
        for j in range(-1, L - 1):
            h = hdnn.layer(j, h)[1]  # the device's own last hidden rows
        xd = torch.from_numpy(x).cuda()
        dense = torch.empty((n, O), dtype=torch.float32, device="cuda")
        for kind in ("shared", "utterances"):
            sr, sp, nd = tables(kind, n, O, np.random.default_rng(n))
            ndd = torch.from_numpy(nd).cuda()
            probs, inact = torch.empty(n * SET_LEN, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
            runs = {"dense": lambda: hdnn.calculateDevice(xd.data_ptr(), n, dense.data_ptr(), s),
                    "sets": lambda: hdnn.calculateLazySetsDevice(xd.data_ptr(), n, sr, sp, ndd.data_ptr(), probs.data_ptr(), inact.data_ptr(), s)}
            runs["sets"]()
            torch.cuda.synchronize()
            want = [hdnn.setLayer(h[a:b], nd[p:q])[1:] for a, b, p, q in zip(sr, sr[1:], sp, sp[1:])]
            if not (same_bytes(probs.cpu().numpy(), np.concatenate([w[0].ravel() for w in want])) and
                    same_bytes(inact.cpu().numpy(), np.concatenate([w[1] for w in want]))):
                sys.exit(f"half_set_sweep: {kind} n {n}: a set probability differs from the debug layer call on the same rows")
            for f in runs.values():
                for _ in range(3):
                    f()
            us = {k: [] for k in ("dense", "sets", "dense_output", "set_step")}
            reps = max(4, min(50, 20000 // n))
            for _ in range(ROUNDS):
                for k, f in runs.items():
                    us[k].append(timed(f, reps))
                us["dense_output"].append(hdnn.layerMicros(L - 1, h, reps=reps))
                us["set_step"].append(hdnn.setLayerMicros(h, sr, sp, nd, reps=reps))
            st = {k: stats(v) for k, v in us.items()}
            for what, a, b in (("forward", "dense", "sets"), ("output", "dense_output", "set_step")):
                margin = max(st[a]["spread"], st[b]["spread"])
                holds = st[b]["median"] <= st[a]["median"] * (1.0 + margin)
                ok = ok and holds
                results.append({"what": what, "sets": kind, "frames": n, "segments": len(sr) - 1, "dense_us": round(st[a]["median"], 1),
                                "dense_spread": st[a]["spread"], "set_us": round(st[b]["median"], 1), "set_spread": st[b]["spread"],
                                "set_over_dense": round(st[b]["median"] / st[a]["median"], 3), "no_slower": holds})
                print(json.dumps(results[-1]), flush=True)
    print(json.dumps({"condition": "the set form no slower than the dense form at every size, margin the larger spread", "holds": ok}), flush=True)
    hdnn.delete()
    if args.out:
        json.dump(results, open(args.out, "w"), indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
