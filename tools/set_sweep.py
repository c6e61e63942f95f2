"""Lazy output for a shared node set against the list path and the bit-mask path, on the same active set (fdnn_set.hip vs
fdnn_lists.hip vs the masked output kernels).

Device-resident, the full 432 -> 7x2048 -> 8000 net: the hidden layers run once per batch size, then per set length the
three output paths are timed over the same context and the same set (one set of `len` nodes, drawn uniformly without
replacement, shared by every row),
  set    fdnn_ctx_lazy_output_set_device         (MFMA kernel forced: fdnn_debug_set_kernel(1); + one wave per row)
  lists  fdnn_ctx_lazy_output_lists_device       (the set repeated per row; score kernel over the entries + one wave per row)
  bits   fdnn_ctx_lazy_output_batch_bits_device  (whole output layer, masked in the epilogue, soft-max scale)
alternated in one process: warm-up, then ROUNDS blocks per path of `reps` calls between two device events; the figure is the
median block's time per call, the spread its (max - min) / median.  A path WINS over another where its slowest block beats
the other's fastest block; anything else is a tie inside the blocks' spread.

  python tools/set_sweep.py [--batches 8,100,1000,10000] [--lens 8,80,400,1600,3200] [--out FILE.json]

Prints one JSON line per (batch, len), the table, and per shape which paths the set path wins over."""
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


def reps_for(n):
    return 200 if n <= 100 else 100 if n <= 1000 else 20


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="8,100,1000,10000")
    ap.add_argument("--lens", default="8,80,400,1600,3200")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batches = [int(v) for v in args.batches.split(",")]
    lens = [int(v) for v in args.lens.split(",")]
    path = F.ensure_model_file(os.path.join(os.environ.get("TMPDIR", "/tmp"), "fdnn_net_seed1_gauss.bin"), F.NET_TOPOLOGY, seed=1, mode="gauss")
    dnn = api.QuantizedDnn.loadFromFile(path)
    O = dnn.outputDimension()
    api.set_kernel(1)
    s = torch.cuda.current_stream().cuda_stream
    results = []
    for n in batches:
        x = torch.from_numpy(F.synth_features(n, dnn.inputDimension(), seed=500 + n)).cuda()
        ctx = dnn.getNewLazyContext(n)
        ctx.calculateUntilOutputDevice(x.data_ptr(), s)
        d_out = torch.empty((n, O), dtype=torch.float32, device="cuda")
        for length in lens:
            nodes = np.sort(np.random.default_rng(n + length).choice(O, length, replace=False)).astype(np.int32)
            nnz = n * length
            mask = np.zeros((1, O), np.int8)
            mask[0, nodes] = 1
            d_set = torch.from_numpy(nodes).cuda()
            d_rp = torch.arange(n + 1, dtype=torch.int32, device="cuda") * length
            d_nd = d_set.repeat(n)
            d_bits = torch.from_numpy(F.pack_mask_bits(mask).view(np.int64)).cuda().repeat(n, 1).contiguous()
            d_p = torch.empty(nnz, dtype=torch.float32, device="cuda")   # the set path's probs [n][len]
            d_lp = torch.empty(nnz, dtype=torch.float32, device="cuda")  # the list path's
            d_i, d_li = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
            runs = {"set": lambda: ctx.calculateForOutputNodeSetDevice(d_set.data_ptr(), length, d_p.data_ptr(), d_i.data_ptr(), 0, n, s),
                    "lists": lambda: ctx.calculateForOutputNodesListsDevice(d_rp.data_ptr(), d_nd.data_ptr(), nnz, d_lp.data_ptr(), d_li.data_ptr(), 0, n, s),
                    "bits": lambda: ctx.calculateForOutputNodesBatchBitsDevice(d_bits.data_ptr(), d_out.data_ptr(), 0, n, s)}
            for _ in range(3):  # warm-up, all paths
                for f in runs.values():
                    f()
            torch.cuda.synchronize()
            # set and lists: the same bytes; bits: another summation order, the project's 2e-6 bar
            assert torch.equal(d_p.view(torch.int32), d_lp.view(torch.int32)) and torch.equal(d_i.view(torch.int32), d_li.view(torch.int32)), \
                f"n {n} len {length}: the set path's bytes differ from the list path's"
            diff = float((d_out[:, d_set.long()].reshape(-1) - d_p).abs().max())
            assert diff <= 2e-6, f"n {n} len {length}: the set path and the bit-mask path differ by {diff}"
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
            rec = {"frames": n, "len": length, "nnz": nnz, "reps": reps, "max_abs_diff_bits": diff}
            for k, v in us.items():
                rec[k + "_us"] = round(float(np.median(v)), 2)
                rec[k + "_min_us"], rec[k + "_max_us"] = round(min(v), 2), round(max(v), 2)
                rec[k + "_spread"] = round((max(v) - min(v)) / float(np.median(v)), 3)
            rec["wins_over"] = [k for k in ("lists", "bits") if rec["set_max_us"] < rec[k + "_min_us"]]
            rec["loses_to"] = [k for k in ("lists", "bits") if rec["set_min_us"] > rec[k + "_max_us"]]
            results.append(rec)
            print(json.dumps(rec), flush=True)
            d_set = d_rp = d_nd = d_bits = d_p = d_lp = d_i = d_li = None
        ctx.delete()
        d_out = x = None
    api.set_kernel(0)
    print("\n| frames | len | set us | lists us | bits us | lists / set | bits / set | spread set / lists / bits | set wins over | set loses to |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        print(f"| {r['frames']} | {r['len']} | {r['set_us']} | {r['lists_us']} | {r['bits_us']} | {r['lists_us'] / r['set_us']:.2f} | "
              f"{r['bits_us'] / r['set_us']:.2f} | {r['set_spread']} / {r['lists_spread']} / {r['bits_spread']} | "
              f"{', '.join(r['wins_over']) or '-'} | {', '.join(r['loses_to']) or '-'} |")
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    dnn.delete()
    return 0


if __name__ == "__main__":
    sys.exit(main())
