"""Lazy output for per-utterance node sets: ONE segmented call (fdnn_sets.hip) against one set call per utterance
(fdnn_set.hip) and against the bit-mask path on the same batch.

Device-resident, the full 432 -> 7x2048 -> 8000 net: S utterances of `frames` frames in one context, each with its own set of
`len` nodes (drawn uniformly without replacement); the hidden layers run once per S, then the three output paths are timed
over the same context,
  sets   one fdnn_ctx_lazy_output_sets_device call with S segments
  set    S fdnn_ctx_lazy_output_set_device calls on the same stream, one per utterance's row range
  bits   fdnn_ctx_lazy_output_batch_bits_device on the whole batch (the sets as masks; whole output layer)
alternated in one process (MFMA kernel forced: fdnn_debug_set_kernel(1)): warm-up, then ROUNDS blocks per path of `reps`
repetitions between two device events; the figure is the median block's time per repetition, the spread its
(max - min) / median.  A path WINS over another where its slowest block beats the other's fastest block.

  python tools/sets_sweep.py [--shapes 1x80,4x80,16x80,64x80,16x8,16x800] [--frames 100] [--out FILE.json]

Prints one JSON line per shape and the table.  (The serving half of the comparison is tools/serve_bench.cpp: modes set,
setserver, and lazy / lazyserver with SET_LEN.)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fast_dnn_amd import api  # noqa: E402
from fast_dnn_amd import formats as F  # noqa: E402

ROUNDS = 5


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="1x80,4x80,16x80,64x80,16x8,16x800", help="S x len, comma separated")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in sh.split("x")) for sh in args.shapes.split(",")]
    path = F.ensure_model_file(os.path.join(os.environ.get("TMPDIR", "/tmp"), "fdnn_net_seed1_gauss.bin"), F.NET_TOPOLOGY, seed=1, mode="gauss")
    dnn = api.QuantizedDnn.loadFromFile(path)
    O = dnn.outputDimension()
    api.set_kernel(1)
    s = torch.cuda.current_stream().cuda_stream
    fr = args.frames
    results = []
    for S, length in shapes:
        n = S * fr
        x = torch.from_numpy(F.synth_features(n, dnn.inputDimension(), seed=700 + n)).cuda()
        ctx = dnn.getNewLazyContext(n)
        ctx.calculateUntilOutputDevice(x.data_ptr(), s)
        rng = np.random.default_rng(S * 1000 + length)
        sets = [np.sort(rng.choice(O, length, replace=False)).astype(np.int32) for _ in range(S)]
        seg_rows = (np.arange(S + 1) * fr).astype(np.int32)
        set_ptr = (np.arange(S + 1) * length).astype(np.int32)
        masks = np.zeros((n, O), np.int8)
        for u, nd in enumerate(sets):
            masks[u * fr:(u + 1) * fr, nd] = 1
        d_nodes = torch.from_numpy(np.concatenate(sets)).cuda()
        d_bits = torch.from_numpy(F.pack_mask_bits(masks).view(np.int64)).cuda()
        nnz = n * length
        d_p, d_sp = torch.empty(nnz, dtype=torch.float32, device="cuda"), torch.empty(nnz, dtype=torch.float32, device="cuda")
        d_i, d_si = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
        d_out = torch.empty((n, O), dtype=torch.float32, device="cuda")

        def per_utterance():
            for u in range(S):
                ctx.calculateForOutputNodeSetDevice(d_nodes.data_ptr() + 4 * u * length, length, d_sp.data_ptr() + 4 * u * fr * length,
                                                    d_si.data_ptr() + 4 * u * fr, u * fr, fr, s)

        runs = {"sets": lambda: ctx.calculateForOutputNodeSetsDevice(seg_rows, set_ptr, d_nodes.data_ptr(), d_p.data_ptr(), d_i.data_ptr(), s),
                "set": per_utterance,
                "bits": lambda: ctx.calculateForOutputNodesBatchBitsDevice(d_bits.data_ptr(), d_out.data_ptr(), 0, n, s)}
        before = api.sets_launches()
        for _ in range(3):  # warm-up, all paths
            for f in runs.values():
                f()
        torch.cuda.synchronize()
        launches = sum(api.sets_launches()[:2]) - sum(before[:2])
        assert launches == 3 * -(-S // 64), f"S {S}: {launches} launches of the segmented kernel in 3 calls"
        # sets and set: the same bytes; bits: another summation order, the project's 2e-6 bar
        assert torch.equal(d_p.view(torch.int32), d_sp.view(torch.int32)) and torch.equal(d_i.view(torch.int32), d_si.view(torch.int32)), \
            f"S {S} len {length}: the segmented call's bytes differ from the per-utterance calls'"
        listed = torch.from_numpy(masks != 0).cuda()
        diff = float((d_out[listed] - d_p).abs().max())
        assert diff <= 2e-6, f"S {S} len {length}: the set path and the bit-mask path differ by {diff}"
        reps = max(5, args.reps // max(1, S // 4))
        us = {k: [] for k in runs}
        for _ in range(ROUNDS):
            for k, f in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    f()
                e1.record()
                e1.synchronize()
                us[k].append(1000.0 * e0.elapsed_time(e1) / reps)
        rec = {"utterances": S, "frames": fr, "len": length, "nnz": nnz, "reps": reps, "max_abs_diff_bits": diff}
        for k, v in us.items():
            rec[k + "_us"] = round(float(np.median(v)), 2)
            rec[k + "_min_us"], rec[k + "_max_us"] = round(min(v), 2), round(max(v), 2)
            rec[k + "_spread"] = round((max(v) - min(v)) / float(np.median(v)), 3)
        rec["wins_over"] = [k for k in ("set", "bits") if rec["sets_max_us"] < rec[k + "_min_us"]]
        rec["loses_to"] = [k for k in ("set", "bits") if rec["sets_min_us"] > rec[k + "_max_us"]]
        results.append(rec)
        print(json.dumps(rec), flush=True)
        ctx.delete()
        d_nodes = d_bits = d_p = d_sp = d_i = d_si = d_out = x = listed = None
    api.set_kernel(0)
    print("\n| utterances x frames | len | sets us | S x set us | bits us | set / sets | bits / sets | spread sets / set / bits | sets wins over | sets loses to |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        print(f"| {r['utterances']} x {r['frames']} | {r['len']} | {r['sets_us']} | {r['set_us']} | {r['bits_us']} | {r['set_us'] / r['sets_us']:.2f} | "
              f"{r['bits_us'] / r['sets_us']:.2f} | {r['sets_spread']} / {r['set_spread']} / {r['bits_spread']} | "
              f"{', '.join(r['wins_over']) or '-'} | {', '.join(r['loses_to']) or '-'} |")
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    dnn.delete()
    return 0


if __name__ == "__main__":
    sys.exit(main())
