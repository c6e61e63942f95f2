"""The top-k selection kernel (fdnn_topk.hip) against two yardsticks on the same device rows: a device-to-device copy of the
rows (twice the bytes the resident form must read) and torch.topk on the same tensor.

Device-resident soft-max-like rows [n][width] (width 8000, and one width just past the resident limit); per (n, k) the
selection is timed in both forms,
  resident   fdnn_topk_rows_device under fdnn_debug_set_topk_kernel(1)   (the row kept in LDS; widths up to the limit)
  streaming  fdnn_topk_rows_device under fdnn_debug_set_topk_kernel(2)   (the passes re-read the row)
  copy       torch's device-to-device copy of the rows
  torch      torch.topk(rows, k, dim=1, sorted=True)
alternated in one process: warm-up, then ROUNDS blocks per path of `reps` calls between two device events; the figure is the
median block's time per call, the spread its (max - min) / median.  Before timing, both forms' bytes are compared with each
other and, on rows without ties, the nodes with torch.topk's.

  python tools/topk_sweep.py [--widths 8000,16385] [--batches 100,1000,10000] [--ks 1,8,32,128,256] [--out FILE.json]

Prints one JSON line per (width, n, k) and the table."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fast_dnn_amd import api  # noqa: E402

ROUNDS = 5


def reps_for(n, width):
    return 200 if n * width <= 1_000_000 else 50 if n * width <= 10_000_000 else 10


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--widths", default=f"8000,{api.TOPK_RESIDENT_WIDTH + 1}")
    ap.add_argument("--batches", default="100,1000,10000")
    ap.add_argument("--ks", default="1,8,32,128,256")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    s = torch.cuda.current_stream().cuda_stream
    results = []
    for width in [int(v) for v in args.widths.split(",")]:
        for n in [int(v) for v in args.batches.split(",")]:
            g = torch.Generator(device="cuda").manual_seed(width + n)
            rows = torch.softmax(torch.randn((n, width), generator=g, device="cuda") * 3.0, dim=1).contiguous()
            dst = torch.empty_like(rows)
            for k in [int(v) for v in args.ks.split(",")]:
                dn = [torch.empty((n, k), dtype=torch.int32, device="cuda") for _ in range(2)]
                dv = [torch.empty((n, k), dtype=torch.float32, device="cuda") for _ in range(2)]

                def select(mode, slot):
                    api.set_topk_kernel(mode)
                    api.topk_rows_device(rows.data_ptr(), n, width, k, dn[slot].data_ptr(), dv[slot].data_ptr(), s)

                runs = {"streaming": lambda: select(2, 1), "copy": lambda: dst.copy_(rows), "torch": lambda: torch.topk(rows, k, dim=1, sorted=True)}
                if width <= api.TOPK_RESIDENT_WIDTH:
                    runs = {"resident": lambda: select(1, 0), **runs}
                for _ in range(3):
                    for f in runs.values():
                        f()
                torch.cuda.synchronize()
                if "resident" in runs:
                    assert torch.equal(dn[0], dn[1]) and torch.equal(dv[0].view(torch.int32), dv[1].view(torch.int32)), "the two forms' bytes differ"
                tv, ti = torch.topk(rows, k, dim=1, sorted=True)
                assert torch.equal(tv.view(torch.int32), dv[1].view(torch.int32)), "values differ from torch.topk's"
                distinct = (tv[:, 1:] != tv[:, :-1]).all(dim=1) if k > 1 else torch.ones(n, dtype=torch.bool, device="cuda")
                assert torch.equal(ti[distinct].int(), dn[1][distinct]), "nodes differ from torch.topk's on rows without ties"
                reps = reps_for(n, width)
                us = {name: [] for name in runs}
                for _ in range(ROUNDS):
                    for name, f in runs.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(reps):
                            f()
                        e1.record()
                        e1.synchronize()
                        us[name].append(1000.0 * e0.elapsed_time(e1) / reps)
                rec = {"width": width, "frames": n, "k": k, "reps": reps, "row_mb": round(n * width * 4 / 1e6, 2)}
                for name, v in us.items():
                    rec[name + "_us"] = round(float(np.median(v)), 2)
                    rec[name + "_spread"] = round((max(v) - min(v)) / float(np.median(v)), 3)
                results.append(rec)
                print(json.dumps(rec), flush=True)
            rows = dst = None
    api.set_topk_kernel(0)
    print("\n| width | frames | k | resident us | streaming us | copy us | torch.topk us | resident / copy | spread res / str / copy / torch |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in results:
        res = r.get("resident_us")
        print(f"| {r['width']} | {r['frames']} | {r['k']} | {res if res is not None else '-'} | {r['streaming_us']} | {r['copy_us']} | {r['torch_us']} | "
              f"{(res / r['copy_us']) if res is not None else float('nan'):.2f} | "
              f"{r.get('resident_spread', '-')} / {r['streaming_spread']} / {r['copy_spread']} / {r['torch_spread']} |")
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
