"""The half-precision net on the device (fdnn_half.hip), measured -- the method of tools/float_sweep.py:
  layers   hgemm_kernel alone per layer shape of the bench net (fdnn_debug_half_layer_us; the output layer's figure includes
           the soft-max scale pass): microseconds, TF/s (2 n K rows FLOP over that time) and the share of the fp16 MFMA peak
           (v_mfma_f32_32x32x16_f16: 32768 FLOP per 32 cycles and SIMD = 4096 FLOP per clock and CU)
  forward  fdnn_half_calculate_device beside fdnn_float_calculate_device and fdnn_calculate_device on the same frames:
           alternated in one process, warm-up, then ROUNDS blocks each; the median block, the spread (max - min) / median
  trace    per-launch kernel times from a rocprofv3 run of its own:
               rocprofv3 --kernel-trace --output-format csv -d DIR -o k -- python tools/half_sweep.py --trace-run 10000
               python tools/half_sweep.py --trace DIR --frames 10000
           the launches of a pass are matched to the layers by their order behind the input step; TF/s from the shapes.

  small    the small-batch kernel (fdnn_half_small.hip; setSmall) beside the tiled one on the same model at 1 .. 128 frames:
           per layer shape and for the forward, alternated block by block in one process, with the quantized scorer's forward;
           beside each layer the time to stream its weights once at the HBM peak (bench.py's roofline figure).  The leg ends
           with the condition of DESIGN section 33: small no slower than tiled by more than the larger spread, at every n.
               python tools/half_sweep.py --small [--batches 1,10,32,100,128]

  mid      the mid-batch kernel (fdnn_half_mid.hip; setMid) beside the tiled one on the same model at 129 .. 4096 frames:
           first the two forwards' bytes must be equal; then per layer shape (with the share of the fp16 MFMA peak) and for
           the forward, alternated block by block in one process.  The leg ends with the condition of DESIGN section 35: mid
           no slower than tiled by more than the larger spread at every n up to 1000; larger n are reported.
               python tools/half_sweep.py --mid [--batches 129,256,512,1000,2048,4096]

  large    the large-batch kernel (fdnn_half_large.hip; setLarge) beside the tiled one on the same model: first the two forwards'
           bytes must be equal; then per layer shape at --layer-batches (one chunk each) and the forward at --batches, with the
           share of the fp16 MFMA peak, setLarge(0) and setLarge(1) alternated block by block in one process.  The leg ends
           with the condition of DESIGN section 36: the hidden form and the forward no slower than tiled by more than the
           larger spread at every size; layer 0 and the output form are reported the same way.
               python tools/half_sweep.py --large [--layer-batches 1808,2048,4096] [--batches 4096,10000,20480]

  python tools/half_sweep.py [--batches 1000,10000] [--out FILE.json]"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fast_dnn_amd import api  # noqa: E402
from fast_dnn_amd import formats as F  # noqa: E402

ROUNDS = 5
CHUNK = 4096  # the nets' default chunk
FLOP_PER_CLOCK_CU = 4096.0
HBM_PEAK_GBS = 8000.0  # bench.py's roofline figure
SMALL_BATCHES = "1,10,32,100,128"
MID_BATCHES = "129,256,512,1000,2048,4096"
LARGE_LAYER_BATCHES = "1808,2048,4096"  # the tail chunk of a 10 000-frame call, half a chunk, a chunk
LARGE_BATCHES = "4096,10000,20480"


def stats(v):
    med = float(np.median(v))
    return {"median": med, "spread": round((max(v) - min(v)) / med, 3)}


def timed(f, reps):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    e1.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / reps  # microseconds per call


def model_path():
    return F.ensure_model_file(os.path.join(os.environ.get("TMPDIR", "/tmp"), "fdnn_net_seed1_gauss.bin"), F.NET_TOPOLOGY, seed=1, mode="gauss")


def peak_tflops():
    import torch

    p = torch.cuda.get_device_properties(0)
    khz = getattr(p, "clock_rate", 2400000)  # (kHz; the MI355X's 2.4 GHz where the binding does not say)
    return FLOP_PER_CLOCK_CU * p.multi_processor_count * khz * 1e3 / 1e12, p.multi_processor_count, khz / 1e6


def trace_run(n):
    import torch

    hdnn = api.HalfDnn.loadFromFile(model_path())
    x = torch.from_numpy(F.synth_features(n, hdnn.inputDimension(), seed=500 + n)).cuda()
    out = torch.empty((n, hdnn.outputDimension()), dtype=torch.float32, device="cuda")
    for _ in range(8):
        hdnn.calculateDevice(x.data_ptr(), n, out.data_ptr(), 0)
    torch.cuda.synchronize()
    hdnn.delete()


def trace_digest(directory, n):
    files = glob.glob(directory + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        sys.exit("half_sweep: no *kernel_trace.csv under " + directory)
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    topo = list(F.NET_TOPOLOGY)
    topo[0] = -(-topo[0] // 4) * 4
    chunks = [min(CHUNK, n - f) for f in range(0, n, CHUNK)]
    groups, idx, passes = {}, 0, -1
    for r in rows:
        if "input_step" in r["Kernel_Name"]:
            idx, passes = 0, passes + 1
        elif "hgemm_kernel" in r["Kernel_Name"]:
            groups.setdefault((idx, chunks[passes % len(chunks)]), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            idx += 1
    print("| layer | frames | K x rows | launches | us mean | min | max | TF/s |\n|---|---|---|---|---|---|---|---|")
    for (j, m), v in sorted(groups.items()):
        v = v[len(v) // 2:]  # the first half is warm-up
        mean = sum(v) / len(v)
        print(f"| {j} | {m} | {topo[j]} x {topo[j + 1]} | {len(v)} | {mean:.1f} | {min(v):.1f} | {max(v):.1f} | {2.0 * m * topo[j] * topo[j + 1] / mean / 1e6:.0f} |")


def small_leg(batches, out):
    import torch

    path = model_path()
    hdnn, qdnn = api.HalfDnn.loadFromFile(path), api.QuantizedDnn.loadFromFile(path)
    D, O, L = hdnn.inputDimension(), hdnn.outputDimension(), hdnn.layerCount()
    s = torch.cuda.current_stream().cuda_stream
    shapes = {"layer0": (0, D, hdnn.layerDimension(0)), "hidden": (1, hdnn.layerDimension(0), hdnn.layerDimension(1)),
              "output": (L - 1, hdnn.layerDimension(L - 2), O)}
    forms = {"tiled": 0, "small": 128}
    results, ok = [], True
    for n in batches:
        rng = np.random.default_rng(n)
        ins = {k: (F.synth_features(n, D, seed=500 + n) if k == "layer0" else rng.random((n, K), dtype=np.float32)) for k, (_, K, _) in shapes.items()}
        us = {(k, f): [] for k in shapes for f in forms}
        for _ in range(ROUNDS):
            for k, (j, _, _) in shapes.items():
                for f, setting in forms.items():
                    hdnn.setSmall(setting)
                    us[k, f].append(hdnn.layerMicros(j, ins[k], reps=20))
        for k, (j, K, rows) in shapes.items():
            st = {f: stats(us[k, f]) for f in forms}
            results.append({"what": "layer", "layer": k, "frames": n, "K": K, "rows": rows, "tiled_us": round(st["tiled"]["median"], 1),
                            "tiled_spread": st["tiled"]["spread"], "small_us": round(st["small"]["median"], 1), "small_spread": st["small"]["spread"],
                            "weights_at_hbm_peak_us": round(2.0 * K * rows / HBM_PEAK_GBS / 1e3, 2)})
            print(json.dumps(results[-1]), flush=True)
        x = torch.from_numpy(ins["layer0"]).cuda()
        outs = {k: torch.empty((n, O), dtype=torch.float32, device="cuda") for k in ("tiled", "small", "quantized")}

        def half(form):
            hdnn.setSmall(forms[form])
            hdnn.calculateDevice(x.data_ptr(), n, outs[form].data_ptr(), s)

        runs = {"tiled": lambda: half("tiled"), "small": lambda: half("small"),
                "quantized": lambda: qdnn.calculate_device(x.data_ptr(), n, outs["quantized"].data_ptr(), s)}
        for f in runs.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        if not torch.equal(outs["tiled"].view(torch.int32), outs["small"].view(torch.int32)):
            sys.exit(f"half_sweep: the small form's bytes differ from the tiled form's at n = {n}")
        us = {k: [] for k in runs}
        for _ in range(ROUNDS):
            for k, f in runs.items():
                us[k].append(timed(f, 20))
        st = {k: stats(us[k]) for k in runs}
        margin = max(st["tiled"]["spread"], st["small"]["spread"])
        holds = st["small"]["median"] <= st["tiled"]["median"] * (1.0 + margin)
        ok = ok and holds
        results.append({"what": "forward", "frames": n, **{k + "_us": round(st[k]["median"], 1) for k in runs}, **{k + "_spread": st[k]["spread"] for k in runs},
                        "small_no_slower": holds})
        print(json.dumps(results[-1]), flush=True)
    print("\n| frames | layer | K x rows | tiled us | spread | small us | spread | weights at HBM peak us |\n|---|---|---|---|---|---|---|---|")
    for r in results:
        if r["what"] == "layer":
            print(f"| {r['frames']} | {r['layer']} | {r['K']} x {r['rows']} | {r['tiled_us']} | {r['tiled_spread']} | {r['small_us']} | {r['small_spread']} | {r['weights_at_hbm_peak_us']} |")
    print("\n| frames | tiled us | spread | small us | spread | quantized us | spread | small no slower |\n|---|---|---|---|---|---|---|---|")
    for r in results:
        if r["what"] == "forward":
            print(f"| {r['frames']} | {r['tiled_us']} | {r['tiled_spread']} | {r['small_us']} | {r['small_spread']} | {r['quantized_us']} | {r['quantized_spread']} | {r['small_no_slower']} |")
    if out:
        with open(out, "w") as fh:
            json.dump(results, fh, indent=1)
    hdnn.delete()
    qdnn.delete()
    return 0 if ok else 1


def mid_leg(batches, out):
    import torch

    hdnn = api.HalfDnn.loadFromFile(model_path())
    D, O, L = hdnn.inputDimension(), hdnn.outputDimension(), hdnn.layerCount()
    peak, cus, ghz = peak_tflops()
    print(json.dumps({"what": "peak", "fp16_mfma_tflops": round(peak, 1), "cus": cus, "ghz": ghz}), flush=True)
    s = torch.cuda.current_stream().cuda_stream
    shapes = {"layer0": (0, D, hdnn.layerDimension(0)), "hidden": (1, hdnn.layerDimension(0), hdnn.layerDimension(1)),
              "output": (L - 1, hdnn.layerDimension(L - 2), O)}
    forms = {"tiled": 0, "mid": 4096}
    results, ok = [], True

    def holds(st):  # mid no slower than tiled by more than the larger of the two spreads
        return st["mid"]["median"] <= st["tiled"]["median"] * (1.0 + max(st["tiled"]["spread"], st["mid"]["spread"]))

    for n in batches:
        rng = np.random.default_rng(n)
        ins = {k: (F.synth_features(n, D, seed=500 + n) if k == "layer0" else rng.random((n, K), dtype=np.float32)) for k, (_, K, _) in shapes.items()}
        x = torch.from_numpy(ins["layer0"]).cuda()
        outs = {f: torch.empty((n, O), dtype=torch.float32, device="cuda") for f in forms}

        def forward(form):
            hdnn.setMid(forms[form])
            hdnn.calculateDevice(x.data_ptr(), n, outs[form].data_ptr(), s)

        for f in forms:
            for _ in range(3):
                forward(f)
        torch.cuda.synchronize()
        if not torch.equal(outs["tiled"].view(torch.int32), outs["mid"].view(torch.int32)):
            sys.exit(f"half_sweep: the mid form's bytes differ from the tiled form's at n = {n}")
        us = {(k, f): [] for k in shapes for f in forms}
        for _ in range(ROUNDS):
            for k, (j, _, _) in shapes.items():
                for f, setting in forms.items():
                    hdnn.setMid(setting)
                    us[k, f].append(hdnn.layerMicros(j, ins[k], reps=20))
        for k, (j, K, rows) in shapes.items():
            st = {f: stats(us[k, f]) for f in forms}
            good = holds(st)
            ok = ok and (good or n > 1000)
            share = {f: round(2.0 * n * K * rows / st[f]["median"] / 1e6 / peak, 3) for f in forms}
            results.append({"what": "layer", "layer": k, "frames": n, "K": K, "rows": rows, "tiled_us": round(st["tiled"]["median"], 1),
                            "tiled_spread": st["tiled"]["spread"], "mid_us": round(st["mid"]["median"], 1), "mid_spread": st["mid"]["spread"],
                            "tiled_of_peak": share["tiled"], "mid_of_peak": share["mid"], "mid_no_slower": good})
            print(json.dumps(results[-1]), flush=True)
        fus = {f: [] for f in forms}
        for _ in range(ROUNDS):
            for f in forms:
                fus[f].append(timed(lambda: forward(f), 20))
        st = {f: stats(fus[f]) for f in forms}
        good = holds(st)
        ok = ok and (good or n > 1000)
        results.append({"what": "forward", "frames": n, **{f + "_us": round(st[f]["median"], 1) for f in forms}, **{f + "_spread": st[f]["spread"] for f in forms},
                        "mid_frames_per_s": round(n / st["mid"]["median"] * 1e6), "mid_no_slower": good})
        print(json.dumps(results[-1]), flush=True)
    print("\n| frames | layer | K x rows | tiled us | spread | of peak | mid us | spread | of peak | mid no slower |\n|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        if r["what"] == "layer":
            print(f"| {r['frames']} | {r['layer']} | {r['K']} x {r['rows']} | {r['tiled_us']} | {r['tiled_spread']} | {r['tiled_of_peak']} | {r['mid_us']} | {r['mid_spread']} | {r['mid_of_peak']} | {r['mid_no_slower']} |")
    print("\n| frames | tiled us | spread | mid us | spread | mid frames/s | mid no slower |\n|---|---|---|---|---|---|---|")
    for r in results:
        if r["what"] == "forward":
            print(f"| {r['frames']} | {r['tiled_us']} | {r['tiled_spread']} | {r['mid_us']} | {r['mid_spread']} | {r['mid_frames_per_s']} | {r['mid_no_slower']} |")
    print("\nthe condition (mid no slower than tiled at every size up to 1000 frames, per layer and for the forward):", "holds" if ok else "FAILS")
    if out:
        with open(out, "w") as fh:
            json.dump(results, fh, indent=1)
    hdnn.setMid(0)
    hdnn.delete()
    return 0 if ok else 1


def large_leg(layer_batches, batches, out):
    import torch

    hdnn = api.HalfDnn.loadFromFile(model_path())
    D, O, L = hdnn.inputDimension(), hdnn.outputDimension(), hdnn.layerCount()
    peak, cus, ghz = peak_tflops()
    print(json.dumps({"what": "peak", "fp16_mfma_tflops": round(peak, 1), "cus": cus, "ghz": ghz}), flush=True)
    s = torch.cuda.current_stream().cuda_stream
    shapes = {"layer0": (0, D, hdnn.layerDimension(0)), "hidden": (1, hdnn.layerDimension(0), hdnn.layerDimension(1)),
              "output": (L - 1, hdnn.layerDimension(L - 2), O)}
    forms = {"tiled": 0, "large": 1}
    flop_per_frame = 2.0 * sum(K * rows for K, rows in zip([D] + [hdnn.layerDimension(j) for j in range(L - 1)], [hdnn.layerDimension(j) for j in range(L)]))
    results, ok = [], True

    def row(st, n, flop, extra):  # large no slower than tiled by more than the larger of the two spreads
        good = st["large"]["median"] <= st["tiled"]["median"] * (1.0 + max(st["tiled"]["spread"], st["large"]["spread"]))
        r = {"frames": n, **extra, **{f + "_us": round(st[f]["median"], 1) for f in forms}, **{f + "_spread": st[f]["spread"] for f in forms},
             **{f + "_of_peak": round(flop / st[f]["median"] / 1e6 / peak, 3) for f in forms}, "large_no_slower": good}
        results.append(r)
        print(json.dumps(r), flush=True)
        return good

    for n in batches:  # the forwards first: their bytes must be equal before anything is timed
        x = torch.from_numpy(F.synth_features(n, D, seed=500 + n)).cuda()
        outs = {f: torch.empty((n, O), dtype=torch.float32, device="cuda") for f in forms}

        def forward(form):
            hdnn.setLarge(forms[form])
            hdnn.calculateDevice(x.data_ptr(), n, outs[form].data_ptr(), s)

        for f in forms:
            for _ in range(3):
                forward(f)
        torch.cuda.synchronize()
        if not torch.equal(outs["tiled"].view(torch.int32), outs["large"].view(torch.int32)):
            sys.exit(f"half_sweep: the large form's bytes differ from the tiled form's at n = {n}")
        fus = {f: [] for f in forms}
        for _ in range(ROUNDS):
            for f in forms:
                fus[f].append(timed(lambda: forward(f), 20))
        st = {f: stats(fus[f]) for f in forms}
        ok = row(st, n, flop_per_frame * n, {"what": "forward", "large_frames_per_s": round(n / st["large"]["median"] * 1e6)}) and ok
    for n in layer_batches:
        rng = np.random.default_rng(n)
        ins = {k: (F.synth_features(n, D, seed=500 + n) if k == "layer0" else rng.random((n, K), dtype=np.float32)) for k, (_, K, _) in shapes.items()}
        us = {(k, f): [] for k in shapes for f in forms}
        for _ in range(ROUNDS):
            for k, (j, _, _) in shapes.items():
                for f, setting in forms.items():
                    hdnn.setLarge(setting)
                    us[k, f].append(hdnn.layerMicros(j, ins[k], reps=20))
        for k, (j, K, rows) in shapes.items():
            good = row({f: stats(us[k, f]) for f in forms}, n, 2.0 * n * K * rows, {"what": "layer", "layer": k, "K": K, "rows": rows})
            ok = ok and (good or k != "hidden")
    head = "tiled us | spread | of peak | large us | spread | of peak | large no slower |"
    print("\n| frames | layer | K x rows | " + head + "\n|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        if r["what"] == "layer":
            print(f"| {r['frames']} | {r['layer']} | {r['K']} x {r['rows']} | {r['tiled_us']} | {r['tiled_spread']} | {r['tiled_of_peak']} | {r['large_us']} | {r['large_spread']} | {r['large_of_peak']} | {r['large_no_slower']} |")
    print("\n| frames | " + head + " large frames/s |\n|---|---|---|---|---|---|---|---|---|")
    for r in results:
        if r["what"] == "forward":
            print(f"| {r['frames']} | {r['tiled_us']} | {r['tiled_spread']} | {r['tiled_of_peak']} | {r['large_us']} | {r['large_spread']} | {r['large_of_peak']} | {r['large_no_slower']} | {r['large_frames_per_s']} |")
    print("\nthe condition (the hidden form and the forward no slower than tiled at every size):", "holds" if ok else "FAILS")
    if out:
        with open(out, "w") as fh:
            json.dump(results, fh, indent=1)
    hdnn.setLarge(0)
    hdnn.delete()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default=None, help="frame counts (default 1000,10000; with --small " + SMALL_BATCHES + ")")
    ap.add_argument("--small", action="store_true", help="the small-batch kernel beside the tiled one at 1 .. 128 frames")
    ap.add_argument("--mid", action="store_true", help="the mid-batch kernel beside the tiled one at 129 .. 4096 frames")
    ap.add_argument("--large", action="store_true", help="the large-batch kernel beside the tiled one")
    ap.add_argument("--layer-batches", default=LARGE_LAYER_BATCHES, help="with --large: frame counts of the per-layer rows")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", type=int, default=0, help="only run 8 forwards of this many frames (under rocprofv3)")
    ap.add_argument("--trace", default=None, help="digest the kernel trace under this directory")
    ap.add_argument("--frames", type=int, default=10000, help="frames of the traced forwards")
    args = ap.parse_args()
    if args.trace:
        return trace_digest(args.trace, args.frames)
    if args.trace_run:
        return trace_run(args.trace_run)
    if args.small:
        return small_leg([int(v) for v in (args.batches or SMALL_BATCHES).split(",")], args.out)
    if args.mid:
        return mid_leg([int(v) for v in (args.batches or MID_BATCHES).split(",")], args.out)
    if args.large:
        return large_leg([int(v) for v in args.layer_batches.split(",")], [int(v) for v in (args.batches or LARGE_BATCHES).split(",")], args.out)
    import torch

    path = model_path()
    nets = {"float": api.FloatDnn.loadFromFile(path), "half": api.HalfDnn.loadFromFile(path), "quantized": api.QuantizedDnn.loadFromFile(path)}
    hdnn = nets["half"]
    D, O, L = hdnn.inputDimension(), hdnn.outputDimension(), hdnn.layerCount()
    peak, cus, ghz = peak_tflops()
    print(json.dumps({"what": "peak", "fp16_mfma_tflops": round(peak, 1), "cus": cus, "ghz": ghz}), flush=True)
    s = torch.cuda.current_stream().cuda_stream
    shapes = {"layer0": (0, D, hdnn.layerDimension(0)), "hidden": (1, hdnn.layerDimension(0), hdnn.layerDimension(1)),
              "output": (L - 1, hdnn.layerDimension(L - 2), O)}
    results = []
    for n in [int(v) for v in (args.batches or "1000,10000").split(",")]:
        rng = np.random.default_rng(n)
        ins = {k: (F.synth_features(n, D, seed=500 + n) if k == "layer0" else rng.random((n, K), dtype=np.float32)) for k, (_, K, _) in shapes.items()}
        us = {k: [] for k in shapes}
        for _ in range(ROUNDS):
            for k, (j, _, _) in shapes.items():
                us[k].append(hdnn.layerMicros(j, ins[k], reps=10))
        for k, (j, K, rows) in shapes.items():
            st = stats(us[k])
            tf = 2.0 * n * K * rows / st["median"] / 1e6
            results.append({"what": "layer", "layer": k, "frames": n, "K": K, "rows": rows, "us": round(st["median"], 1), "spread": st["spread"],
                            "tflops": round(tf, 1), "of_peak": round(tf / peak, 3)})
            print(json.dumps(results[-1]), flush=True)
        x = torch.from_numpy(ins["layer0"]).cuda()
        outs = {k: torch.empty((n, O), dtype=torch.float32, device="cuda") for k in nets}
        runs = {"float": lambda: nets["float"].calculateDevice(x.data_ptr(), n, outs["float"].data_ptr(), s),
                "half": lambda: hdnn.calculateDevice(x.data_ptr(), n, outs["half"].data_ptr(), s),
                "quantized": lambda: nets["quantized"].calculate_device(x.data_ptr(), n, outs["quantized"].data_ptr(), s)}
        reps = {"float": 3, "half": 10, "quantized": 20}
        for f in runs.values():
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        us = {k: [] for k in runs}
        for _ in range(ROUNDS):
            for k, f in runs.items():
                us[k].append(timed(f, reps[k]))
        for k in runs:
            st = stats(us[k])
            results.append({"what": "forward", "net": k, "frames": n, "us": round(st["median"], 1), "spread": st["spread"],
                            "frames_per_s": round(n / st["median"] * 1e6)})
            print(json.dumps(results[-1]), flush=True)
    print("\n| frames | layer | K x rows | us | TF/s | of peak | spread |\n|---|---|---|---|---|---|---|")
    for r in results:
        if r["what"] == "layer":
            print(f"| {r['frames']} | {r['layer']} | {r['K']} x {r['rows']} | {r['us']} | {r['tflops']} | {r['of_peak']} | {r['spread']} |")
    print("\n| frames | net | us | frames/s | spread |\n|---|---|---|---|---|")
    for r in results:
        if r["what"] == "forward":
            print(f"| {r['frames']} | {r['net']} | {r['us']} | {r['frames_per_s']} | {r['spread']} |")
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    for d in nets.values():
        d.delete()
    return 0


if __name__ == "__main__":
    sys.exit(main())
