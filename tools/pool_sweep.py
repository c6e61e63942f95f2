"""The class-pooling kernel (fdnn_pool.hip) against two yardsticks on the same device rows: a device-to-device copy of the
rows (twice the bytes the resident form must read) and the same sums by torch (index_add_ over the transposed rows, and a
one-hot fp32 matmul).

Device-resident soft-max-like rows [n][width] (width 8000, and one width just past the resident limit); per (n, C, map) the
pooling is timed in both forms,
  resident   fdnn_pool_rows_device under fdnn_debug_set_pool_kernel(1)   (the row kept in LDS; widths up to the limit)
  streaming  fdnn_pool_rows_device under fdnn_debug_set_pool_kernel(2)   (members gathered from memory)
  copy       torch's device-to-device copy of the rows
  index_add  out.zero_(); out.index_add_(1, class_of, rows)
  matmul     rows @ onehot [width][C], fp32
alternated in one process: warm-up, then ROUNDS blocks per path of `reps` calls between two device events; the figure is the
median block's time per call, the spread its (max - min) / median.  Before timing, both forms' bytes are compared with each
other and with the host restatement (api.pool_ref) on the first rows, and torch's sums to the derived bound.

  python tools/pool_sweep.py [--widths 8000,16385] [--batches 100,1000,10000] [--classes 2,48,1000,0] [--out FILE.json]

(0 classes = the identity map, C = width.)  Prints one JSON line per (width, n, C, map) and the table."""
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
    ap.add_argument("--widths", default=f"8000,{api.POOL_RESIDENT_WIDTH + 1}")
    ap.add_argument("--batches", default="100,1000,10000")
    ap.add_argument("--classes", default="2,48,1000,0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    s = torch.cuda.current_stream().cuda_stream
    results = []
    for width in [int(v) for v in args.widths.split(",")]:
        for n in [int(v) for v in args.batches.split(",")]:
            g = torch.Generator(device="cuda").manual_seed(width + n)
            rows = torch.softmax(torch.randn((n, width), generator=g, device="cuda") * 3.0, dim=1).contiguous()
            dst = torch.empty_like(rows)
            head = rows[:4].cpu().numpy()
            for C in [int(v) or width for v in args.classes.split(",")]:
                for kind in (("interleaved", "block") if C < width else ("identity",)):
                    i = np.arange(width, dtype=np.int64)
                    co = (i % C if kind != "block" else np.minimum(i * C // width, C - 1)).astype(np.int32)
                    pool = api.ClassPool(co, C)
                    dq = [torch.empty((n, C), dtype=torch.float32, device="cuda") for _ in range(2)]
                    d_co = torch.from_numpy(co.astype(np.int64)).cuda()
                    out_t = torch.empty((n, C), dtype=torch.float32, device="cuda")
                    onehot = torch.zeros((width, C), dtype=torch.float32, device="cuda") if width * C <= 64_000_000 else None
                    if onehot is not None:
                        onehot[torch.arange(width, device="cuda"), d_co] = 1.0

                    def run_pool(mode, slot):
                        api.set_pool_kernel(mode)
                        pool.rows_device(rows.data_ptr(), n, dq[slot].data_ptr(), s)

                    def index_add():
                        out_t.zero_()
                        out_t.index_add_(1, d_co, rows)

                    runs = {"streaming": lambda: run_pool(2, 1), "copy": lambda: dst.copy_(rows), "index_add": index_add}
                    if onehot is not None:
                        runs["matmul"] = lambda: torch.matmul(rows, onehot)
                    if width <= api.POOL_RESIDENT_WIDTH:
                        runs = {"resident": lambda: run_pool(1, 0), **runs}
                    for _ in range(3):
                        for f in runs.values():
                            f()
                    torch.cuda.synchronize()
                    if "resident" in runs:
                        assert torch.equal(dq[0].view(torch.int32), dq[1].view(torch.int32)), "the two forms' bytes differ"
                    want = api.pool_ref(head, co, C)
                    assert np.array_equal(dq[1][:4].cpu().numpy().view(np.uint32), want.view(np.uint32)), "bytes differ from the host restatement"
                    size = np.bincount(co, minlength=C).astype(np.float64)
                    d = np.ceil(size / api.POOL_LANES) + 4
                    slack = torch.from_numpy((2 * d * 2.0 ** -24)[None, :]).cuda() * dq[1].double() + 1e-30  # both sums within their bound
                    assert ((out_t.double() - dq[1].double()).abs() <= slack + size.max() * 2.0 ** -24 * dq[1].double()).all(), "torch's sums are elsewhere"
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
                    rec = {"width": width, "frames": n, "classes": C, "map": kind, "reps": reps, "row_mb": round(n * width * 4 / 1e6, 2)}
                    for name, v in us.items():
                        rec[name + "_us"] = round(float(np.median(v)), 2)
                        rec[name + "_spread"] = round((max(v) - min(v)) / float(np.median(v)), 3)
                    results.append(rec)
                    print(json.dumps(rec), flush=True)
                    pool.delete()
                    onehot = None
            rows = dst = None
    api.set_pool_kernel(0)
    print("\n| width | frames | C | map | resident us | streaming us | copy us | index_add us | matmul us | resident / copy | spread res / str / copy |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        res = r.get("resident_us")
        print(f"| {r['width']} | {r['frames']} | {r['classes']} | {r['map']} | {res if res is not None else '-'} | {r['streaming_us']} | {r['copy_us']} | "
              f"{r['index_add_us']} | {r.get('matmul_us', '-')} | {(res / r['copy_us']) if res is not None else float('nan'):.2f} | "
              f"{r.get('resident_spread', '-')} / {r['streaming_spread']} / {r['copy_spread']} |")
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
