"""Lazy output by active-node lists against the bit-mask path, on the same active sets (fdnn_lists.hip vs the masked output kernels).

Device-resident, the full 432 -> 7x2048 -> 8000 net: the hidden layers run once per batch size, then per active share the
two output paths are timed over the same context and the same sets,
  lists  fdnn_ctx_lazy_output_lists_device       (score kernel over the entries + one wave per row)
  bits   fdnn_ctx_lazy_output_batch_bits_device  (whole output layer, masked in the epilogue, soft-max scale)
A/B-alternated in one process: warm-up, then ROUNDS blocks per path of `reps` calls between two device events; the figure is
the median block's time per call, the spread its (max - min) / median.  Active sets: per row `round(share * O)` nodes (at
least one), drawn uniformly without replacement, independently per row (no frame-to-frame coherence: the gather's worst case).
The crossover per batch size is the largest share at which the list path is still the faster one.

  python tools/lists_sweep.py [--batches 1,8,100,1000,10000] [--shares 0.0005,0.001,0.01,0.05,0.1,0.4] [--out FILE.json]

Prints one JSON line per (batch, share), the table, the crossovers and the verdict on the one acceptance bar: at 0.1 % over
10 000 frames the list path's slowest block must beat the bit-mask path's fastest block."""
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


def active_sets(n, O, share, seed):
    """-> (row_ptr, nodes, bits): k = max(1, round(share * O)) nodes per row, uniform without replacement, ascending."""
    k = max(1, int(round(share * O)))
    rng = np.random.default_rng(seed)
    nodes = np.empty((n, k), np.int32)
    for lo in range(0, n, 1000):  # (blocks: the random matrix of 10 000 x 8000 stays small)
        r = rng.random((min(1000, n - lo), O), dtype=np.float32)
        nodes[lo:lo + r.shape[0]] = np.sort(np.argpartition(r, k - 1, axis=1)[:, :k], axis=1)
    masks = np.zeros((n, O), np.int8)
    masks[np.arange(n)[:, None], nodes] = 1
    row_ptr = (np.arange(n + 1, dtype=np.int64) * k).astype(np.int32)
    return row_ptr, nodes.reshape(-1), F.pack_mask_bits(masks)


def reps_for(n):
    return 200 if n <= 100 else 100 if n <= 1000 else 20


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="1,8,100,1000,10000")
    ap.add_argument("--shares", default="0.0005,0.001,0.01,0.05,0.1,0.4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batches = [int(v) for v in args.batches.split(",")]
    shares = [float(v) for v in args.shares.split(",")]
    path = F.ensure_model_file(os.path.join(os.environ.get("TMPDIR", "/tmp"), "fdnn_net_seed1_gauss.bin"), F.NET_TOPOLOGY, seed=1, mode="gauss")
    dnn = api.QuantizedDnn.loadFromFile(path)
    O = dnn.outputDimension()
    s = torch.cuda.current_stream().cuda_stream
    results = []
    for n in batches:
        x = torch.from_numpy(F.synth_features(n, dnn.inputDimension(), seed=500 + n)).cuda()
        ctx = dnn.getNewLazyContext(n)
        ctx.calculateUntilOutputDevice(x.data_ptr(), s)
        d_out = torch.empty((n, O), dtype=torch.float32, device="cuda")
        for share in shares:
            row_ptr, nodes, bits = active_sets(n, O, share, seed=n + int(share * 1e5))
            nnz = int(row_ptr[-1])
            d_rp, d_nd = torch.from_numpy(row_ptr).cuda(), torch.from_numpy(nodes).cuda()
            d_bits = torch.from_numpy(bits.view(np.int64)).cuda()
            d_p = torch.empty(nnz, dtype=torch.float32, device="cuda")
            d_i = torch.empty(n, dtype=torch.float32, device="cuda")
            runs = {"lists": lambda: ctx.calculateForOutputNodesListsDevice(d_rp.data_ptr(), d_nd.data_ptr(), nnz, d_p.data_ptr(), d_i.data_ptr(), 0, n, s),
                    "bits": lambda: ctx.calculateForOutputNodesBatchBitsDevice(d_bits.data_ptr(), d_out.data_ptr(), 0, n, s)}
            for _ in range(3):  # warm-up, both paths
                for f in runs.values():
                    f()
            torch.cuda.synchronize()
            # the same numbers from both paths (different summation orders: the project's 2e-6 bar)
            rows = torch.from_numpy(np.repeat(np.arange(n), np.diff(row_ptr))).cuda()
            diff = float((d_out[rows, d_nd.long()] - d_p).abs().max())
            assert diff <= 2e-6, f"n {n} share {share}: the paths differ by {diff}"
            rows = None
            reps = reps_for(n)
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
            rec = {"frames": n, "share": share, "per_row": nnz // n, "nnz": nnz, "reps": reps, "max_abs_diff": diff}
            for k, v in us.items():
                rec[k + "_us"] = round(float(np.median(v)), 2)
                rec[k + "_min_us"], rec[k + "_max_us"] = round(min(v), 2), round(max(v), 2)
                rec[k + "_spread"] = round((max(v) - min(v)) / float(np.median(v)), 3)
            rec["weight_bytes_listed"] = nnz * 2048
            rec["speedup"] = round(rec["bits_us"] / rec["lists_us"], 2)
            results.append(rec)
            print(json.dumps(rec), flush=True)
            d_rp = d_nd = d_bits = d_p = d_i = None
        ctx.delete()
        d_out = x = None
    print("\n| frames | share | per row | lists us | bits us | bits / lists | spread lists / bits |")
    print("|---|---|---|---|---|---|---|")
    for r in results:
        print(f"| {r['frames']} | {100 * r['share']:g} % | {r['per_row']} | {r['lists_us']} | {r['bits_us']} | {r['speedup']} | {r['lists_spread']} / {r['bits_spread']} |")
    print()
    for n in batches:
        won = [r["share"] for r in results if r["frames"] == n and r["lists_max_us"] < r["bits_min_us"]]
        print(f"crossover, {n} frames: the list path is faster up to {100 * max(won):g} % active" if won else f"crossover, {n} frames: the list path is never faster")
    bar = [r for r in results if r["frames"] == 10000 and abs(r["share"] - 0.001) < 1e-9]
    ok = None
    if bar:
        ok = bar[0]["lists_max_us"] < bar[0]["bits_min_us"]
        print(f"acceptance (0.1 % over 10 000 frames): lists {bar[0]['lists_us']} us (max {bar[0]['lists_max_us']}) vs bits {bar[0]['bits_us']} us "
              f"(min {bar[0]['bits_min_us']}): {'FASTER' if ok else 'NOT FASTER'}")
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    dnn.delete()
    return 0 if ok in (None, True) else 1


if __name__ == "__main__":
    sys.exit(main())
