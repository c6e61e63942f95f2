"""Lazy output by lists over per-frame-group node unions against the dot-product lists and the bit-mask path, on the same
active sets (fdnn_lists_union.hip vs fdnn_lists.hip vs the masked output kernels).

Device-resident, the full 432 -> 7x2048 -> 8000 net: the hidden layers run once per batch size, then per (share, churn) the
paths are timed over the same context and the same sets,
  union.gG  fdnn_ctx_lazy_output_lists_device with fdnn_model_set_lists_union(G), G in --groups
  lists     fdnn_ctx_lazy_output_lists_device with the switch at 0 (one 16-lane dot product per entry)
  bits      fdnn_ctx_lazy_output_batch_bits_device (whole output layer, masked in the epilogue, soft-max scale)
alternated in one process: warm-up, then ROUNDS blocks per path of `reps` calls between two device events (reps sized from
the warm-up so that a block runs about BLOCK_MS); the figure is the median block's time per call, the spread its
(max - min) / median.  A path WINS over another where its slowest block beats the other's fastest block.

Active sets: `round(share * O)` nodes per row (at least one).  churn 0: every row the same set; churn c in (0, 1): FuncTest's
model as formats.generate_masks states it -- every frame int(O * c) inactive nodes come on and as many active ones go off
(a share of the LAYER, not of the set: at 5 % active and c = 0.03 more than half of a row's nodes are new); churn 1:
independent sets per row.  The union columns give the mean union length over the mean row length per group size.

  python tools/lists_union_sweep.py [--batches 100,1000,10000] [--shares 0.001,0.01,0.05,0.1,0.2,0.4] [--churns 0,0.03,1]
                                    [--groups 1,2,4,8] [--out FILE.json]

Prints one JSON line per (batch, share, churn), the table, and which group size is the best at 5 % / churn 0.03 / the largest batch."""
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
BLOCK_MS = 50.0


def active_masks(n, O, share, churn, seed):
    """-> masks [n][O] int8 with k = max(1, round(share * O)) ones per row (see the module text for churn)."""
    k = max(1, int(round(share * O)))
    rng = np.random.default_rng(seed)
    masks = np.zeros((n, O), np.int8)
    if churn >= 1.0:
        for lo in range(0, n, 1000):  # (blocks: the random matrix of 10 000 x 8000 stays small)
            r = rng.random((min(1000, n - lo), O), dtype=np.float32)
            idx = np.argpartition(r, k - 1, axis=1)[:, :k]
            masks[np.arange(lo, lo + r.shape[0])[:, None], idx] = 1
        return masks
    row = np.zeros(O, bool)
    row[rng.choice(O, k, replace=False)] = True
    new = min(int(O * churn), O - k)
    for f in range(n):
        if f and new:
            row[rng.choice(np.flatnonzero(~row), new, replace=False)] = True
            row[rng.choice(np.flatnonzero(row), new, replace=False)] = False
        masks[f] = row
    return masks


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="100,1000,10000")
    ap.add_argument("--shares", default="0.001,0.01,0.05,0.1,0.2,0.4")
    ap.add_argument("--churns", default="0,0.03,1")
    ap.add_argument("--groups", default="1,2,4,8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batches = [int(v) for v in args.batches.split(",")]
    shares = [float(v) for v in args.shares.split(",")]
    churns = [float(v) for v in args.churns.split(",")]
    groups = [int(v) for v in args.groups.split(",")]
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
            for churn in churns:
                masks = active_masks(n, O, share, churn, seed=n + int(share * 1e5) + int(churn * 100))
                row_ptr, nodes = F.masks_to_lists(masks)
                bits = F.pack_mask_bits(masks)
                masks = None
                nnz = int(row_ptr[-1])
                union_x = {g: round(float(api.lists_union_ref(row_ptr, nodes, O, g)[0].mean()) / (nnz / n), 2) for g in groups}
                d_rp, d_nd = torch.from_numpy(row_ptr).cuda(), torch.from_numpy(nodes).cuda()
                d_bits = torch.from_numpy(bits.view(np.int64)).cuda()
                d_p = torch.empty(nnz, dtype=torch.float32, device="cuda")   # the dot-product lists' probs
                d_up = torch.empty(nnz, dtype=torch.float32, device="cuda")  # the union path's
                d_i, d_ui = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")

                def lists_call(g, probs, inactive):
                    dnn.setListsUnion(g)
                    ctx.calculateForOutputNodesListsDevice(d_rp.data_ptr(), d_nd.data_ptr(), nnz, probs.data_ptr(), inactive.data_ptr(), 0, n, s)

                runs = {f"union.g{g}": (lambda g=g: lists_call(g, d_up, d_ui)) for g in groups}
                runs["lists"] = lambda: lists_call(0, d_p, d_i)
                runs["bits"] = lambda: ctx.calculateForOutputNodesBatchBitsDevice(d_bits.data_ptr(), d_out.data_ptr(), 0, n, s)
                # warm-up, every path; the union path's bytes are the dot-product lists' for every group size
                est = {}
                for k, f in runs.items():
                    f()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    f()
                    e1.record()
                    e1.synchronize()
                    est[k] = e0.elapsed_time(e1) / 2
                    if k.startswith("union"):
                        if "lists" not in est:
                            runs["lists"]()
                            torch.cuda.synchronize()
                        assert torch.equal(d_up.view(torch.int32), d_p.view(torch.int32)) and torch.equal(d_ui.view(torch.int32), d_i.view(torch.int32)), \
                            f"n {n} share {share} churn {churn} {k}: the union path's bytes differ from the dot-product lists'"
                        d_up.zero_()
                rows = torch.from_numpy(np.repeat(np.arange(n), np.diff(row_ptr))).cuda()
                diff = float((d_out[rows, d_nd.long()] - d_p).abs().max())
                assert diff <= 2e-6, f"n {n} share {share} churn {churn}: lists and bits differ by {diff}"
                rows = None
                reps = {k: int(min(200, max(2, round(BLOCK_MS / max(v, 1e-3))))) for k, v in est.items()}
                us = {k: [] for k in runs}
                for _ in range(ROUNDS):
                    for k, f in runs.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(reps[k]):
                            f()
                        e1.record()
                        e1.synchronize()
                        us[k].append(1000.0 * e0.elapsed_time(e1) / reps[k])
                dnn.setListsUnion(0)
                rec = {"frames": n, "share": share, "churn": churn, "per_row": round(nnz / n, 1), "nnz": nnz, "max_abs_diff_bits": diff,
                       "union_over_row": {f"g{g}": union_x[g] for g in groups}}
                for k, v in us.items():
                    rec[k + "_us"] = round(float(np.median(v)), 2)
                    rec[k + "_min_us"], rec[k + "_max_us"] = round(min(v), 2), round(max(v), 2)
                    rec[k + "_spread"] = round((max(v) - min(v)) / float(np.median(v)), 3)
                    rec[k + "_reps"] = reps[k]
                best = min((f"union.g{g}" for g in groups), key=lambda k: rec[k + "_us"])
                rec["best_union"] = best
                rec["wins_over"] = [k for k in ("lists", "bits") if rec[best + "_max_us"] < rec[k + "_min_us"]]
                rec["loses_to"] = [k for k in ("lists", "bits") if rec[best + "_min_us"] > rec[k + "_max_us"]]
                results.append(rec)
                print(json.dumps(rec), flush=True)
                d_rp = d_nd = d_bits = d_p = d_up = d_i = d_ui = None
        ctx.delete()
        d_out = x = None
    head = " | ".join(f"union g{g} us" for g in groups)
    print(f"\n| frames | share | churn | per row | union / row (g{groups[0]} .. g{groups[-1]}) | {head} | lists us | bits us | best union wins over | loses to |")
    print("|" + "---|" * (9 + len(groups)))
    for r in results:
        ux = " ".join(f"{r['union_over_row'][f'g{g}']:g}" for g in groups)
        cols = " | ".join(str(r[f"union.g{g}_us"]) for g in groups)
        print(f"| {r['frames']} | {100 * r['share']:g} % | {r['churn']:g} | {r['per_row']:g} | {ux} | {cols} | {r['lists_us']} | {r['bits_us']} | "
              f"{', '.join(r['wins_over']) or '-'} | {', '.join(r['loses_to']) or '-'} |")
    bar = [r for r in results if r["frames"] == max(batches) and abs(r["share"] - 0.05) < 1e-9 and abs(r["churn"] - 0.03) < 1e-9]
    if bar:
        print(f"\nbest group size at 5 % / churn 0.03 / {max(batches)} frames: {bar[0]['best_union']} "
              f"({bar[0][bar[0]['best_union'] + '_us']} us; lists {bar[0]['lists_us']} us, bits {bar[0]['bits_us']} us)")
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    dnn.delete()
    return 0


if __name__ == "__main__":
    sys.exit(main())
