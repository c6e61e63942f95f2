"""The unquantized net on the device (fdnn_float.hip), measured: per layer shape of the bench net and per batch size,
  layers   fgemm_kernel alone (fdnn_debug_float_layer_us: one upload, a warm-up run, then runs back to back between two device
           events; the output layer's figure includes the soft-max scale pass): microseconds and TF/s (2 n K rows FLOP over
           that time; a batch above 4096 frames runs as chunks, the last one a partial round of tiles)
  forward  fdnn_float_calculate_device, whole net, frames/s -- beside the quantized scorer's fdnn_calculate_device on the same
           frames and the numpy path of `tools/accuracy_report.py --host` (convert.float_forward, 200 frames)
  report   fdnn_report_add_device: GB/s over the 2 n O floats it reads
alternated in one process: warm-up, then ROUNDS blocks per item; the figure is the median block, the spread (max - min) / median.

  python tools/float_sweep.py [--batches 1000,10000] [--out FILE.json]

Prints one JSON line per measurement and the tables."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fast_dnn_amd import api, convert as CV  # noqa: E402
from fast_dnn_amd import formats as F  # noqa: E402

ROUNDS = 5


def stats(v):
    med = float(np.median(v))
    return {"median": med, "min": float(min(v)), "max": float(max(v)), "spread": round((max(v) - min(v)) / med, 3)}


def timed(f, reps):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    e1.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / reps  # microseconds per call


def main():
    import torch

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="1000,10000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    batches = [int(v) for v in args.batches.split(",")]
    path = F.ensure_model_file(os.path.join(os.environ.get("TMPDIR", "/tmp"), "fdnn_net_seed1_gauss.bin"), F.NET_TOPOLOGY, seed=1, mode="gauss")
    fdnn = api.FloatDnn.loadFromFile(path)
    qdnn = api.QuantizedDnn.loadFromFile(path)
    D, O, L = fdnn.inputDimension(), fdnn.outputDimension(), fdnn.layerCount()
    s = torch.cuda.current_stream().cuda_stream
    shapes = {"layer0": (0, D, fdnn.layerDimension(0)), "hidden": (1, fdnn.layerDimension(0), fdnn.layerDimension(1)),
              "output": (L - 1, fdnn.layerDimension(L - 2), O)}
    results = []
    for n in batches:
        rng = np.random.default_rng(n)
        ins = {k: (F.synth_features(n, D, seed=500 + n) if k == "layer0" else rng.random((n, K), dtype=np.float32)) for k, (_, K, _) in shapes.items()}
        us = {k: [] for k in shapes}
        for _ in range(ROUNDS):
            for k, (j, _, _) in shapes.items():
                us[k].append(fdnn.layerMicros(j, ins[k], reps=10 if n <= 1000 else 4))  # (each call: its own warm-up run first)
        for k, (j, K, rows) in shapes.items():
            st = stats(us[k])
            rec = {"what": "layer", "layer": k, "frames": n, "K": K, "rows": rows, "us": round(st["median"], 1), "spread": st["spread"],
                   "tflops": round(2.0 * n * K * rows / st["median"] / 1e6, 1)}
            results.append(rec)
            print(json.dumps(rec), flush=True)
        x = torch.from_numpy(ins["layer0"]).cuda()
        d_ref = torch.empty((n, O), dtype=torch.float32, device="cuda")
        d_q = torch.empty((n, O), dtype=torch.float32, device="cuda")
        rep = api.AccuracyReport(O)
        runs = {"float": lambda: fdnn.calculateDevice(x.data_ptr(), n, d_ref.data_ptr(), s),
                "quantized": lambda: qdnn.calculate_device(x.data_ptr(), n, d_q.data_ptr(), s),
                "report": lambda: rep.addDevice(d_ref.data_ptr(), d_q.data_ptr(), n, s)}
        reps = {"float": 3, "quantized": 20, "report": 20}
        for f in runs.values():
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        us = {k: [] for k in runs}
        for _ in range(ROUNDS):
            for k, f in runs.items():
                us[k].append(timed(f, reps[k]))
        for k in ("float", "quantized"):
            st = stats(us[k])
            rec = {"what": "forward", "net": k, "frames": n, "us": round(st["median"], 1), "spread": st["spread"],
                   "frames_per_s": round(n / st["median"] * 1e6)}
            results.append(rec)
            print(json.dumps(rec), flush=True)
        st = stats(us["report"])
        rec = {"what": "report", "frames": n, "O": O, "us": round(st["median"], 1), "spread": st["spread"],
               "gb_per_s": round(2.0 * n * O * 4 / st["median"] / 1e3, 1), "figures": rep.read(0.1)}
        results.append(rec)
        print(json.dumps(rec), flush=True)
        rep.delete()
        x = d_ref = d_q = None
    # the numpy path on this box's CPU
    net = F.read_model_bin(path)
    xh = F.synth_features(200, D, seed=3)
    CV.float_forward(net, xh[:8])
    t0 = time.perf_counter()
    CV.float_forward(net, xh)
    rec = {"what": "forward", "net": "numpy", "frames": 200, "frames_per_s": round(200 / (time.perf_counter() - t0))}
    results.append(rec)
    print(json.dumps(rec), flush=True)
    print("\n| frames | layer | K x rows | us | TF/s | spread |\n|---|---|---|---|---|---|")
    for r in results:
        if r["what"] == "layer":
            print(f"| {r['frames']} | {r['layer']} | {r['K']} x {r['rows']} | {r['us']} | {r['tflops']} | {r['spread']} |")
    print("\n| frames | net | us | frames/s | spread |\n|---|---|---|---|---|")
    for r in results:
        if r["what"] == "forward":
            print(f"| {r['frames']} | {r['net']} | {r.get('us', '-')} | {r['frames_per_s']} | {r.get('spread', '-')} |")
    print("\n| frames | O | report us | GB/s | spread |\n|---|---|---|---|---|")
    for r in results:
        if r["what"] == "report":
            print(f"| {r['frames']} | {r['O']} | {r['us']} | {r['gb_per_s']} | {r['spread']} |")
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    fdnn.delete()
    qdnn.delete()
    return 0


if __name__ == "__main__":
    sys.exit(main())
