"""Raw feature frames spliced on the device against rows spliced on the host (fdnn_splice.hip).

Three legs, each A/B-alternated in one process (the 432 -> 7x2048 -> 8000 net, Kaldi's <Splice> [ -5 .. 5 ] over 39-wide
frames, padded to 432):
  device  fdnn_calculate_raw_device vs fdnn_calculate_device at 10 000 frames, device-resident (ms per pass)
  host    100-frame calls host to host: fdnn_calculate_raw vs fdnn_calculate on host-spliced rows (us per call); the H2D
          bytes per frame are 156 vs 1 728
  serve   16 caller threads x 100-frame utterances through one ScoringServer: submit_raw vs submit (utterances/s)
Every leg first checks that both sides return the same bytes.  --legs device --iters N alone is the rocprofv3 run's
workload (splice_kernel's time: rocprofv3 --kernel-trace --stats -- python tools/splice_bench.py --legs device).

  python tools/splice_bench.py [--legs device,host,serve] [--iters 200] [--seconds 3]
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fast_dnn_amd import api  # noqa: E402
from fast_dnn_amd import convert as CV  # noqa: E402
from fast_dnn_amd import formats as F  # noqa: E402

OFFS, D = list(range(-5, 6)), 39


def raw_frames(n, seed):
    return np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32) * 3


def leg_device(dnn, iters):
    import torch

    n = 10000
    raw = raw_frames(n, 1)
    x = CV.splice_frames(raw, OFFS, dnn.inputDimension())
    d_raw, d_x = torch.from_numpy(raw).cuda(), torch.from_numpy(x).cuda()
    O = dnn.outputDimension()
    a = torch.empty((n, O), dtype=torch.float32, device="cuda")
    b = torch.empty((n, O), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    dnn.calculateRawDevice(d_raw.data_ptr(), n, a.data_ptr(), stream=s)
    dnn.calculate_device(d_x.data_ptr(), n, b.data_ptr(), s)
    torch.cuda.synchronize()
    assert torch.equal(a, b), "raw and spliced passes differ"
    runs = {"raw": lambda: dnn.calculateRawDevice(d_raw.data_ptr(), n, a.data_ptr(), stream=s),
            "spliced": lambda: dnn.calculate_device(d_x.data_ptr(), n, b.data_ptr(), s)}
    ms = {k: [] for k in runs}
    for _ in range(5):  # warm-up
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    for rnd in range(4):  # alternated blocks of iters / 4 passes
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(max(1, iters // 4)):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / max(1, iters // 4))
    return {"leg": "device", "frames": n, "ms_per_pass": {k: [round(v, 4) for v in vs] for k, vs in ms.items()},
            "median_ms": {k: round(float(np.median(vs)), 4) for k, vs in ms.items()},
            "h2d_bytes_per_frame": {"raw": 4 * D, "spliced": 4 * dnn.inputDimension()}}


def leg_host(dnn, iters):
    n = 100
    raws = [raw_frames(n, 10 + i) for i in range(8)]
    xs = [CV.splice_frames(r, OFFS, dnn.inputDimension()) for r in raws]
    outs = [np.empty((n, dnn.outputDimension()), np.float32) for _ in range(2)]
    assert np.array_equal(dnn.calculateRaw(raws[0]), dnn.calculate(xs[0])), "raw and spliced calls differ"
    L, h = api.lib(), dnn.nativeDnnHandle
    c_f = api._c_f32p

    def raw_call(i):
        api._check(L.fdnn_calculate_raw(h, raws[i % 8].ctypes.data_as(c_f), n, D, outs[0].ctypes.data_as(c_f)))

    def spliced_call(i):
        api._check(L.fdnn_calculate(h, xs[i % 8].ctypes.data_as(c_f), n, dnn.inputDimension(), 10, outs[1].ctypes.data_as(c_f)))

    runs = {"raw": raw_call, "spliced": spliced_call}
    for f in runs.values():
        for i in range(20):
            f(i)
    us = {k: [] for k in runs}
    for rnd in range(4):
        for k, f in runs.items():
            t = []
            for i in range(max(1, iters // 4)):
                t0 = time.perf_counter()
                f(i)
                t.append(time.perf_counter() - t0)
            us[k].append(float(np.median(t)) * 1e6)
    return {"leg": "host", "frames_per_call": n, "us_per_call_median_by_block": {k: [round(v, 1) for v in vs] for k, vs in us.items()},
            "median_us": {k: round(float(np.median(vs)), 1) for k, vs in us.items()},
            "h2d_bytes_per_call": {"raw": 4 * D * n, "spliced": 4 * dnn.inputDimension() * n}}


def leg_serve(dnn, seconds, threads=16):
    n = 100
    raws = [raw_frames(n, 100 + i) for i in range(threads)]
    xs = [CV.splice_frames(r, OFFS, dnn.inputDimension()) for r in raws]
    srv = api.ScoringServer(dnn, 4096, 4)
    t, o = srv.submitRaw(raws[0])
    srv.wait(t)
    t2, o2 = srv.submit(xs[0])
    srv.wait(t2)
    assert np.array_equal(o, o2), "raw and spliced submissions differ"
    res = {}
    for rnd in range(2):
        for kind in ("raw", "spliced"):
            stop = time.perf_counter() + seconds
            counts = [0] * threads

            def caller(i):
                out = np.empty((n, dnn.outputDimension()), np.float32)
                while time.perf_counter() < stop:
                    tk, _ = srv.submitRaw(raws[i], out=out) if kind == "raw" else srv.submit(xs[i], out=out)
                    srv.wait(tk)
                    counts[i] += 1

            th = [threading.Thread(target=caller, args=(i,)) for i in range(threads)]
            t0 = time.perf_counter()
            for x in th:
                x.start()
            for x in th:
                x.join()
            res.setdefault(kind, []).append(round(sum(counts) / (time.perf_counter() - t0), 1))
    st = srv.stats()
    srv.close()
    return {"leg": "serve", "threads": threads, "frames_per_utterance": n, "utterances_per_s": res, "server_stats": st}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--legs", default="device,host,serve")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=3.0)
    args = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("splice_bench needs a HIP device")
    import torch  # noqa: F401  (one HIP runtime: torch's, loaded first)

    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "fdnn_net_seed1_gauss.bin")
    F.ensure_model_file(path, F.NET_TOPOLOGY, seed=1, mode="gauss")
    dnn = api.QuantizedDnn.loadFromFile(path, device=0)
    dnn.setSplice(OFFS, D)
    for leg in args.legs.split(","):
        if leg == "device":
            r = leg_device(dnn, args.iters)
        elif leg == "host":
            r = leg_host(dnn, args.iters)
        elif leg == "serve":
            r = leg_serve(dnn, args.seconds)
        else:
            raise SystemExit(f"unknown leg {leg}")
        print(json.dumps(r), flush=True)
    dnn.delete()


if __name__ == "__main__":
    main()
